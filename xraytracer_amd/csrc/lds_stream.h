// lds_stream.h — what the one-wave-per-pixel kernels (pixel.hip, whitted.hip) share: the
// pixel's mt19937 stream in a 624-word circular LDS buffer (x[i] at st[i % 624]; the state
// k_seed wrote is x[0..623]), generated 128 words at a time, and Image::addPixel's ordered sum.
#pragma once
#include "path_common.h"

namespace xrt {

constexpr uint32_t kPixSumStride = 68;             // ordered-sum buffer row (floats): 64 + 4, rows on other banks

// the words generated per chunk: one pair per lane
constexpr uint32_t kPixChunk = 128;

// LDS-fed UniformSampler of one lane: x[c], x[c+1], ... from the wave's circular buffer.  The
// window logic guarantees every word it is asked for has been generated and not overwritten.
struct LdsRng {
    const uint32_t* st;
    uint32_t i;   // c % kMT
    __device__ __forceinline__ float next() {
        const uint32_t y = st[i];
        i = (i + 1 == kMT) ? 0u : i + 1;
        return canonical(mt_temper(y));
    }
};

// x[g .. g+127] into the circular buffer (x[g-624 .. g-1] in it): lane l makes x[g+2l] and
// x[g+2l+1] (libstdc++ _M_gen_rand's recurrence, one word at a time).  Every operand is read
// before any lane writes: lane l's second word needs x[g+2l+2-624], which lane l+1 replaces.
__device__ __forceinline__ void pix_gen(uint32_t* st, uint32_t g, int lane) {
    uint32_t i0 = g % kMT + 2u * (uint32_t)lane;
    if (i0 >= kMT) i0 -= kMT;
    const uint32_t i1 = i0 + 1u;   // g and kMT are even: a pair never wraps
    uint32_t i2 = i1 + 1u;
    if (i2 >= kMT) i2 -= kMT;
    uint32_t j0 = i0 + (kMT - 227u);   // x[i - 227] sits at (i + 397) % 624 (odd: j0 + 1 may wrap)
    if (j0 >= kMT) j0 -= kMT;
    uint32_t j1 = j0 + 1u;
    if (j1 >= kMT) j1 -= kMT;
    const uint32_t a0 = st[i0], a1 = st[i1], a2 = st[i2], b0 = st[j0], b1 = st[j1];
    wave_sync();
    st[i0] = b0 ^ mt_mix(a0, a1);
    st[i1] = b1 ^ mt_mix(a1, a2);
    wave_sync();
}

// Image::addPixel in sample order for the lanes of vm (lane order), each with value r:
// ranked into the sum buffer (3 rows of kPixSumStride floats), then added one after the other
// by lanes 0..2 (a channel each) to their running sum acc.  Every lane of the wave calls it.
__device__ __forceinline__ void pix_add_in_order(float* sum, int lane, float& acc, uint64_t vm, v3 r) {
    if ((vm >> lane) & 1ull) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(vm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)vm, 0u));
        sum[rank] = r.x, sum[kPixSumStride + rank] = r.y, sum[2 * kPixSumStride + rank] = r.z;
    }
    wave_sync();
    if (lane < 3) {
        const float* q = sum + kPixSumStride * lane;
        const f4* q4 = reinterpret_cast<const f4*>(q);
        const uint32_t nv = (uint32_t)__builtin_popcountll(vm);
        uint32_t j = 0;
        for (; j + 8 <= nv; j += 8) {
            const f4 a = q4[j / 4], b = q4[j / 4 + 1];
            acc = acc + a.x, acc = acc + a.y, acc = acc + a.z, acc = acc + a.w;
            acc = acc + b.x, acc = acc + b.y, acc = acc + b.z, acc = acc + b.w;
        }
        for (; j < nv; ++j) acc = acc + q[j];
    }
    wave_sync();   // the buffer is rewritten next time
}

}  // namespace xrt
