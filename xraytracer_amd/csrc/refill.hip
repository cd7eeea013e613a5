// refill.hip — the RNG refill launches every schedule uses.
//
// k_refill_merged: every slot's first twist (the seeding refill after k_seed; later twists
// happen in-line at the end of the step launch a slot runs low in, wave_refill).  Same twist
// as wave_twist (libstdc++ _M_gen_rand: x[g+k] = x[g+k-227] ^ mix(x[g+k-624], x[g+k-623]),
// chunks k = m, 227+m, 454+m held in registers), arranged for bandwidth: the old block is
// staged through LDS (below), the next request's slot, stream position and old block are
// fetched while the current one twists, and the slot state is not touched — the merged
// kernel clears ST_RNGREQ when it first loads the slot, which is always after this kernel.
#include "launch.h"
#include "merged.h"
#include "path_common.h"

namespace xrt {

// CLEAR: also clear the slot's ST_RNGREQ (the wavefront / k_step schedules, whose kernels
// test the flag; the merged kernel clears it itself when it next loads the slot).
template <bool CLEAR>
__global__ __launch_bounds__(kBlock) void k_refill_merged(KParams P, const uint32_t* __restrict__ req,
                                                          const uint32_t* __restrict__ count, uint32_t* zero_count) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[kBlock / 64][2][kMT];
    zero_parts(P, zero_count);
    const PartIter it = part_iter(P, count, kBlock / 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t i = it.first + wv;
    if (i >= it.n) return;
    const uint32_t* rq = req + it.p * P.part_cap;
    uint32_t s = rq[i];
    uint32_t g = glb<gu32>(P.rng_g)[s];
    store_block(load_block(P.ring + (size_t)s * kRing, g, lane), lane, stage[wv][0]);
    for (int buf = 0;; buf ^= 1) {
        // Double-buffered: the next request's old block is in flight (in registers) while
        // this one twists out of LDS.
        const uint32_t in = i + it.stride;
        const bool more = in < it.n;
        uint32_t sn = s, gn = g;
        Staged nx;
        if (more) {
            sn = rq[in];
            gn = glb<gu32>(P.rng_g)[sn];
            nx = load_block(P.ring + (size_t)sn * kRing, gn, lane);
        }
        twist_block(P.ring + (size_t)s * kRing, g, lane, stage[wv][buf]);
        if (lane == 0) {
            P.rng_g[s] = g + kMT;
            if (CLEAR) P.state[s] &= ~ST_RNGREQ;
        }
        if (!more) break;
        store_block(nx, lane, stage[wv][buf ^ 1]);
        s = sn, g = gn, i = in;
    }
}

hipError_t launch_refill_merged(const KParams& P, const uint32_t* count, uint32_t* zero_count, hipStream_t st) {
    // 16384 blocks (64 Ki waves) measured best on C2: 2048 7.7 ms, 4096 6.9, 8192 6.6, 16384 6.5
    // per frame (tools/refill_sweep.sh).
    const uint32_t per = std::max<uint32_t>(1u, std::min<uint32_t>((P.part_cap + 3) / 4, 16384u / P.n_part));
    hipLaunchKernelGGL(k_refill_merged<false>, dim3(P.n_part * per), dim3(kBlock), 0, st, P, P.req, count,
                       zero_count);
    return hipGetLastError();
}

hipError_t launch_refill(const KParams& P, const uint32_t* count, uint32_t* zero_count, hipStream_t st) {
    const uint32_t per = std::max<uint32_t>(1u, std::min<uint32_t>((P.part_cap + 3) / 4, 16384u / P.n_part));
    hipLaunchKernelGGL(k_refill_merged<true>, dim3(P.n_part * per), dim3(kBlock), 0, st, P, P.req, count, zero_count);
    return hipGetLastError();
}

}  // namespace xrt
