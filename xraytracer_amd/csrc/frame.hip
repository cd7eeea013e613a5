// frame.hip — the kernels around a frame's path work, whatever the schedule: k_seed (the
// per-pixel RNG streams and the first slot list), k_finish (the division by the sample count
// and the counter reduction), k_finish_var (a variance render's plane), k_test_slot_map and k_tonemap (gamma and 8-bit quantisation), with their launchers.
#include "launch.h"
#include "path_common.h"

namespace xrt {

// ==================================================================== k_seed ====
// mt19937::seed(j + width*i) for every slot (Src/renderer.cpp:35-36).  The recurrence is
// serial per pixel, so each lane runs one pixel's recurrence and the wave writes the words
// out through an LDS transpose (64 pixels x 64 words, padded row) as coalesced 256-B rows.
__global__ __launch_bounds__(kBlock) void k_seed(KParams P, uint32_t* list, uint32_t* count, uint32_t* count_other,
                                                  uint32_t* req_count) {
    __shared__ uint32_t lds[4][64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t base = (blockIdx.x * kBlock) + wv * 64;
    const uint32_t s = base + lane;
    const bool valid = s < P.n_slots;
    uint32_t row = 0, col = 0;
    if (valid) {
        const SlotPixel pix = slot_pixel(P, s);
        col = pix.col, row = pix.row;
    }
    uint32_t x = col + P.width * row;  // seed j + width * i
    for (uint32_t q = 0; q < kMT; q += 64) {
        for (uint32_t j = 0; j < 64; ++j) {
            const uint32_t i = q + j;
            if (i > 0 && i < kMT) x = 1812433253u * (x ^ (x >> 30)) + i;
            lds[wv][lane][j] = x;
        }
        wave_sync();
        for (uint32_t r = 0; r < 64; ++r) {
            const uint32_t sl = base + r;
            if (sl < P.n_slots && q + lane < kMT) P.ring[(size_t)sl * kRing + q + lane] = lds[wv][r][lane];
        }
        wave_sync();
    }
    if (valid) {
        P.rng_c[s] = kMT;   // cursor: next output is x[624]
        P.rng_g[s] = kMT;   // generated: x[0..623]
        P.state[s] = ST_REGEN | ST_RNGREQ;   // first twist by the k_refill right after
        P.req[s] = s;   // partition p = s / part_cap starts at p * part_cap: identity
        P.sample_k[s] = 0;
        P.depth[s] = 0;
        P.occ[s] = 0;
        P.c_seg[s] = 0;
        P.c_shadow[s] = 0;
        P.c_rej[s] = 0;
        P.c_stall[s] = 0;
        list[s] = s;
    }
    if (blockIdx.x == 0) {
        for (uint32_t p = threadIdx.x; p < P.n_part; p += kBlock) {
            const uint32_t lo = p * P.part_cap;
            const uint32_t c = lo < P.n_slots ? min(P.part_cap, P.n_slots - lo) : 0u;
            count[p] = c;
            count_other[p] = 0;
            req_count[p] = c;
            req_count[kMaxParts + p] = 0;
        }
    }
}

// ================================================================== k_finish ====
// Image::operator/=(Vec3f(n_samples)) over this shard's pixels + counter reduction.
__global__ __launch_bounds__(kBlock) void k_finish(KParams P) {
    SlotCounters cnt;
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < P.n_slots; s += gridDim.x * kBlock) {
        const SlotPixel pix = slot_pixel(P, s);
        const uint32_t col = pix.col, row = pix.row;
        float* px = P.fb + 3 * ((size_t)col + (size_t)P.width * row);
        const v3 mean = frame_mean(mk(px[0], px[1], px[2]), P.spp);
        px[0] = mean.x, px[1] = mean.y, px[2] = mean.z;
        cnt.add(P, s);
    }
    cnt.reduce(P);
}

// ============================================================== k_finish_var ====
// A variance render's plane (xrt_render_var, include/xrt.h) from the slots' {s1, s2} records: the
// variance of the pixel's mean luminance, one rounding per operation.
__global__ __launch_bounds__(kBlock) void k_finish_var(KParams P, const float2* __restrict__ mom, float* __restrict__ var) {
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < P.n_slots; s += gridDim.x * kBlock) {
        const SlotPixel pix = slot_pixel(P, s);
        const uint32_t col = pix.col, row = pix.row;
        var[(size_t)col + (size_t)P.width * row] = frame_variance(mom[s], P.spp);
    }
}

// ============================================================ k_test_slot_map ====
// xrt_test_slot_map: every slot's pixel index, from the function the kernels above and the merged
// schedule's call.
__global__ __launch_bounds__(kBlock) void k_test_slot_map(KParams P, uint32_t* __restrict__ out) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P.n_slots) return;
    const SlotPixel pix = slot_pixel(P, s);
    out[s] = pix.col + P.width * pix.row;
}

// ===================================================================== output ====
// Image::gammaCorrection (Src/image.h:80-90: pow(c, 1.0f / gamma) per channel) followed by
// writePPM's quantisation (:92-114: std::clamp(static_cast<uint32_t>(255.0f * c), 0u, 255u)),
// the float -> uint32 conversion as GCC emits it on x86-64 (a 64-bit truncating convert,
// INT64_MIN for NaN and out-of-range values, low 32 bits kept).  One thread per channel.
__global__ void k_tonemap(const float* __restrict__ rgb, uint32_t n, float inv_gamma, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = 255.0f * glibc_powf(rgb[i], inv_gamma);
    const int64_t q = (v >= -0x1p63f && v < 0x1p63f) ? (int64_t)v : INT64_MIN;
    const uint32_t u = (uint32_t)(uint64_t)q;
    out[i] = (uint8_t)(u < 255u ? u : 255u);
}

hipError_t launch_seed(const KParams& P, uint32_t* list, uint32_t* count, uint32_t* count_other,
                       uint32_t* req_count, hipStream_t st) {
    const uint32_t blocks = (P.n_slots + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_seed, dim3(blocks), dim3(kBlock), 0, st, P, list, count, count_other, req_count);
    return hipGetLastError();
}

hipError_t launch_finish(const KParams& P, hipStream_t st) {
    const uint32_t blocks = std::min<uint32_t>((P.n_slots + kBlock - 1) / kBlock, 2048u);
    hipLaunchKernelGGL(k_finish, dim3(blocks), dim3(kBlock), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_finish_var(const KParams& P, const float2* mom, float* var, hipStream_t st) {
    const uint32_t blocks = std::min<uint32_t>((P.n_slots + kBlock - 1) / kBlock, 2048u);
    hipLaunchKernelGGL(k_finish_var, dim3(blocks), dim3(kBlock), 0, st, P, mom, var);
    return hipGetLastError();
}

hipError_t launch_test_slot_map(const KParams& P, uint32_t* out, hipStream_t st) {
    hipLaunchKernelGGL(k_test_slot_map, dim3((P.n_slots + kBlock - 1) / kBlock), dim3(kBlock), 0, st, P, out);
    return hipGetLastError();
}

hipError_t launch_tonemap(const float* rgb, uint32_t n, float inv_gamma, uint8_t* out, hipStream_t st) {
    hipLaunchKernelGGL(k_tonemap, dim3((n + 255) / 256), dim3(256), 0, st, rgb, n, inv_gamma, out);
    return hipGetLastError();
}

}  // namespace xrt
