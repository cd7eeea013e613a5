// aov.hip — first-hit guide buffers (xrt_render_aov): per pixel the sample means of the first
// hit's albedo, shading normal, depth and coverage, and the object of sample 0, taken through
// the camera rays every schedule builds.
//
// Sample k of pixel (row i, col j) takes words 2k and 2k + 1 of the pixel's mt19937 stream (seed
// j + W * i, k_seed) as its jitter and builds PinholeCamera::sampleRay — bit for bit the camera
// rays of WhittedIntegrator and NormalIntegrator at the same spp.  Each sample is one
// Scene::intersect; nothing else reads the sampler, so the samples of a pixel are independent
// given the stream and the schedule is k_whitted's: one persistent wave per pixel (pixels from
// an atomic counter), the stream in a 624-word LDS ring generated 128 words at a time
// (lds_stream.h), lane l of window w is sample 64 w + l.  There is no ray tree, so no ray ring
// and no per-lane scratch.
//
// Eight float channels per pixel — albedo.rgb, ns.xyz, t, 1 — each start at +0.0f, take every
// sample's value in sample order (a miss adds +0.0f) and are divided once by (float)spp: an
// ordered float sum, as Image::addPixel's, but with no NaN / Inf / negative check (these are
// not radiances).  Lanes 0..7 keep one channel's running sum each.  The wave's LDS slice is
// k_whitted's (kWhitWaveLds: the stream, then 3 * kPixSumStride floats), so a window's values
// pass through it in runs of kAovRun samples: eight rows of kAovRow floats.
//
// Two kernels run this loop: k_aov over a scene resident in LDS (WhitLds), k_aov_bvh over a
// triangle scene beyond LDS through its BVH (WhitBvh); whit_trace.h has both policies.
#include <hip/hip_runtime.h>

#include "whit_trace.h"
#include "launch.h"

namespace xrt {

constexpr uint32_t kAovChannels = 8;
constexpr uint32_t kAovRun = 24;   // samples per pass through the sum buffer
constexpr uint32_t kAovRow = 24;   // row stride (floats): 16-byte rows whose eight readers' f4 loads fall on disjoint banks
static_assert(kAovChannels * kAovRow <= 3 * kPixSumStride, "the eight rows fit k_whitted's sum buffer");
static_assert(kAovRun <= kAovRow && kAovRun % 4 == 0 && kAovRow % 4 == 0, "a run fits a row; f4 reads");

// acc (lanes 0..7: channel `lane`) += v[lane's channel] of lanes 0 .. span - 1, in lane order.
// Every lane of the wave calls it; span is wave-uniform.
__device__ __forceinline__ void aov_add_in_order(float* sum, int lane, float& acc, uint32_t span,
                                                 const float (&v)[kAovChannels]) {
    for (uint32_t b = 0; b < span; b += kAovRun) {
        const uint32_t m = min(kAovRun, span - b);
        const uint32_t r = (uint32_t)lane - b;   // lanes below b wrap far above m
        if (r < m) {
#pragma unroll
            for (uint32_t c = 0; c < kAovChannels; ++c) sum[kAovRow * c + r] = v[c];
        }
        wave_sync();
        if ((uint32_t)lane < kAovChannels) {
            const float* q = sum + kAovRow * (uint32_t)lane;
            if (m == kAovRun) {   // a full run: the loads at once, then the additions in order
                const f4* q4 = reinterpret_cast<const f4*>(q);
                f4 a[kAovRun / 4];
#pragma unroll
                for (uint32_t j = 0; j < kAovRun / 4; ++j) a[j] = q4[j];
#pragma unroll
                for (uint32_t j = 0; j < kAovRun / 4; ++j)
                    acc = acc + a[j].x, acc = acc + a[j].y, acc = acc + a[j].z, acc = acc + a[j].w;
            } else {
                for (uint32_t j = 0; j < m; ++j) acc = acc + q[j];
            }
        }
        wave_sync();   // the buffer is rewritten by the next run
    }
}

// One wave's share of the shard: pixels from the counter at `work` until it runs out (the loop
// of whit_pixels), one Scene::intersect per sample through the trace policy T.
template <typename TR>
__device__ __forceinline__ void aov_pixels(const KParams& P, const AovOut& A, const TR& T, uint32_t* st,
                                           uint32_t* __restrict__ work, int lane) {
    float* sum = reinterpret_cast<float*>(st + kMT);
    const float n = (float)P.spp;
    for (;;) {
        uint32_t s = 0;
        if (lane == 0) s = atomicAdd(work, 1u);
        s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
        if (s >= P.n_slots) break;   // every wave reaches this: the grid drains
        const SlotPixel pix = slot_pixel_rowmajor(P, s);
        const uint32_t col = pix.col, row = pix.row;
        // the seeded state x[0..623] (k_seed) -> the circular buffer, 16 B per lane and load
        {
            const u32x4* src = reinterpret_cast<const u32x4*>(P.ring + (size_t)s * kRing);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if ((uint32_t)lane + 64u * k < kMT / 4) reinterpret_cast<u32x4*>(st)[lane + 64 * k] = src[lane + 64 * k];
            wave_sync();
        }
        float acc = 0.0f;   // lane c < 8: channel c of the running sum
        int first_obj = -1; // lane 0: the object of sample 0
        uint32_t g = kMT;   // x[0 .. g) generated; sample k draws x[kMT + 2k], x[kMT + 2k + 1]
        for (uint32_t k0 = 0; k0 < P.spp; k0 += 64u) {
            const uint32_t span = min(64u, P.spp - k0);
            const uint32_t o = kMT + 2u * k0;
            while (g < o + 2u * span) {   // one chunk per window: g = o before it, o + 128 after
                pix_gen(st, g, lane);
                g += kPixChunk;
            }
            float v[kAovChannels] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if ((uint32_t)lane < span) {
                uint32_t ci = (o % kMT) + 2u * (uint32_t)lane;
                if (ci >= kMT) ci -= kMT;
                LdsRng rng{st, ci};
                const float jx = rng.next();
                const float jy = rng.next();
                v3 ro, rd;
                jitter_ray(P, col, row, jx, jy, ro, rd);
                HitRec h;
                T.closest(ro, rd, h);
                Surf S;
                const int obj = T.surface(ro, rd, h, S);
                if (obj >= 0) {
                    const int mat = T.obj[obj].material;
                    if (mat == XRT_MAT_LAMBERT) {
                        const float* al = A.obj_albedo + 3 * (size_t)obj;
                        v[0] = al[0], v[1] = al[1], v[2] = al[2];
                    } else if (mat == XRT_MAT_METAL || mat == XRT_MAT_GLASS) {
                        v[0] = v[1] = v[2] = 1.0f;
                    }
                    v[3] = S.ns.x, v[4] = S.ns.y, v[5] = S.ns.z;
                    v[6] = h.t;
                    v[7] = 1.0f;
                }
                if (k0 == 0u && lane == 0) first_obj = obj;
            }
            aov_add_in_order(sum, lane, acc, span, v);
        }
        const size_t px = (size_t)col + (size_t)P.width * row;
        const float mean = acc / n;
        if (lane < 3) {
            if (A.albedo) A.albedo[3 * px + lane] = mean;
        } else if (lane < 6) {
            if (A.normal) A.normal[3 * px + (lane - 3)] = mean;
        } else if (lane == 6) {
            if (A.depth) A.depth[px] = mean;
        } else if (lane == 7) {
            if (A.alpha) A.alpha[px] = mean;
        }
        if (lane == 0 && A.object) A.object[px] = first_obj;
        wave_sync();   // the stream buffer is reloaded for the next pixel
    }
}

template <int SCN>
__global__ __launch_bounds__(kWhitBlock) void k_aov(KParams P, AovOut A, uint32_t* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) f4 lds_aov[];
    char* lb = reinterpret_cast<char*>(lds_aov);
    const int tid = threadIdx.x, lane = tid & 63;
    const LScene L = load_lscene(P, lb, tid, kWhitBlock);
    uint32_t* st = reinterpret_cast<uint32_t*>(lb + whit_wave_off(P) + (tid >> 6) * kWhitWaveLds);
    __syncthreads();
    const WhitLds<SCN> T{P, L, L.obj};
    aov_pixels(P, A, T, st, work, lane);
}

template <bool TWO, typename SE>
__global__ __launch_bounds__(kWhitBlock) void k_aov_bvh(KParams P, AovOut A, uint32_t* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) f4 lds_aov_bvh[];
    const auto B = whit_bvh_setup<TWO, SE>(P, reinterpret_cast<char*>(lds_aov_bvh), threadIdx.x);
    aov_pixels(P, A, B.T, B.st, work, threadIdx.x & 63);
}

// one launch over the shard's pixels: a persistent grid, at most one wave per pixel
template <typename K>
static hipError_t aov_launch(K kern, size_t lds, const KParams& P, const AovOut& A, uint32_t* work, hipStream_t st) {
    uint32_t blocks = 0;
    const hipError_t e = persistent_blocks(kern, kWhitBlock, lds, P.n_slots, &blocks);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWhitBlock), lds, st, P, A, work);
    return hipGetLastError();
}

int aov_kernel(const KParams& P) { return use_whitted(P) ? 1 : use_whitted_bvh(P) ? 2 : 0; }

hipError_t launch_aov(const KParams& P, const AovOut& A, uint32_t* work, hipStream_t st) {
    const int which = aov_kernel(P);
    if (!which || !A.obj_albedo) return hipErrorInvalidValue;
    if (hipMemsetAsync(work, 0, sizeof(uint32_t), st) != hipSuccess) return hipErrorInvalidValue;
    if (which == 1)
        return with_scene_kind(P.scene_kind, [&](auto scn) {
            return aov_launch(k_aov<decltype(scn)::value>, whit_lds_bytes(P), P, A, work, st);
        });
    return with_whit_bvh(P, [&](auto two, auto se) {
        return aov_launch(k_aov_bvh<decltype(two)::value, decltype(se)>, whit_bvh_lds_bytes(P), P, A, work, st);
    });
}

}  // namespace xrt
