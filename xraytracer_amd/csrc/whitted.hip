// whitted.hip — WhittedIntegrator (Src/integrator.h:294-398) with the delta lights PointLight /
// DistantLight (Src/light.h:11-49, Src/light.cpp:115-142).
//
// A Whitted sample draws exactly two random words, the pixel jitter (Src/renderer.cpp:44-47):
// nothing the integrator does reads the sampler.  Sample k of a pixel therefore starts at
// stream offset 2k whatever the earlier samples hit, and the samples of a pixel are
// independent given the stream.  One wave takes one pixel (persistent waves take pixels from
// an atomic counter, as k_pixel does) and keeps the pixel's mt19937 stream in a 624-word LDS
// ring, generated 128 words at a time (lds_stream.h).  Lane l of window w is sample
// k = 64 w + l: it reads words 2k and 2k + 1, builds the reference's camera ray and runs the
// whole ray tree of that sample.  The window's radiances pass the renderer's NaN / Inf /
// negative check and three lanes (one per channel) add the accepted ones to the running sum
// in sample order — Image::addPixel's sequence.  No candidate speculation: all 64 lanes of a
// full window are real samples.
//
// The ray tree.  The reference pops a std::queue and adds to total_radiance in pop order,
// i.e. breadth-first order, and float addition is not associative, so that order is part of
// the result.  Each lane keeps the same FIFO: a ring of kWhitQueue = 2^(MAX_DEPTH + 1) rays
// {origin, direction, throughput, depth} in its private (scratch) memory, popped at the head
// and pushed at the tail exactly where the reference pushes (glass: the refracted ray first,
// then the reflected one).  The ring cannot overflow: while the n_d <= 2^d rays of depth d are
// popped, each pushes at most two, so at most n_d - j + 2 j <= 2 n_d <= 2^(d + 1) rays are
// queued after j pops, and the host refuses max_depth > XRT_WHITTED_MAX_DEPTH for scenes that
// hold a glass object; without glass a ray pushes at most one (a chain) and any depth fits.
// Ring indices are masked, so not even a wrong bound could write outside the lane's ring.
//
// All arithmetic is fp32 in the reference's operation order (contraction is off for the
// whole library).  Scalar literals reach the vectors as float (operator*(float, Vec3<T>),
// Src/geometry.h:212-217).  The traces (lscene.h closest_l / occluded_l) take the direction
// as given: a metal child's direction is not normalised, and a NaN direction (normalize of
// refract's zero vector) misses everything, as every `t < best` test fails.
//
// Two kernels run this: k_whitted over a scene resident in LDS, k_whitted_bvh over a triangle
// scene beyond LDS through its BVH (XRT_FLAG_WHITTED_BVH).  They differ in the trace policy
// whit_integrate is instantiated with and in nothing else.
#include <hip/hip_runtime.h>

#include "whit_trace.h"

namespace xrt {

constexpr uint32_t kWhitQueue = 2u << XRT_WHITTED_MAX_DEPTH;          // rays per lane ring (a power of two)
constexpr float kWhitIor = 1.3f;   // Src/integrator.h:359,365: the literal 1.3 bound to `const float& ior`

struct WRay {
    v3 o, d, thr;
    uint32_t depth;
};

// std::clamp(v, lo, hi) (a NaN passes through: both comparisons are false)
__device__ __forceinline__ float whit_clamp(float v, float lo, float hi) { return v < lo ? lo : (hi < v ? hi : v); }

// reflect (Src/geometry.cpp:52-55): I - 2 * dot(I, N) * N
__device__ __forceinline__ v3 whit_reflect(v3 I, v3 N) { return I - N * (2.0f * dot(I, N)); }

// refract (Src/geometry.cpp:57-67); the zero vector when its own k < 0
__device__ __forceinline__ v3 whit_refract(v3 I, v3 N, float ior) {
    float cosi = whit_clamp(dot(I, N), -1.0f, 1.0f);
    float etai = 1.0f, etat = ior;
    v3 n = N;
    if (cosi < 0.0f) {
        cosi = -cosi;
    } else {
        etai = ior, etat = 1.0f;
        n = -N;
    }
    const float eta = etai / etat;
    const float k = 1.0f - eta * eta * (1.0f - cosi * cosi);
    if (k < 0.0f) return mk(0, 0, 0);
    return I * eta + n * (eta * cosi - __builtin_sqrtf(k));
}

// fresnel (Src/geometry.cpp:69-89)
__device__ __forceinline__ float whit_fresnel(v3 I, v3 N, float ior) {
    float cosi = whit_clamp(dot(I, N), -1.0f, 1.0f);
    float etai = 1.0f, etat = ior;
    if (cosi > 0.0f) etai = ior, etat = 1.0f;
    const float sint = etai / etat * __builtin_sqrtf(smax(0.0f, 1.0f - cosi * cosi));
    if (sint >= 1.0f) return 1.0f;
    const float cost = __builtin_sqrtf(smax(0.0f, 1.0f - sint * sint));
    cosi = __builtin_fabsf(cosi);
    const float Rs = ((etat * cosi) - (etai * cost)) / ((etat * cosi) + (etai * cost));
    const float Rp = ((etai * cosi) - (etat * cost)) / ((etai * cosi) + (etat * cost));
    return (Rs * Rs + Rp * Rp) / 2.0f;
}

// per-lane counters of one pixel: Scene::intersect calls, Scene::occluded calls, queue pops,
// depth-overflow pops, glass hits with and without a refracted ray
struct WhitCount {
    uint32_t seg = 0, shadow = 0, rays = 0, cut = 0, refr = 0, tir = 0;
};

// The scene behind whit_integrate is a trace policy (whit_trace.h): closest, occluded, surface
// and the object table `obj`.

// WhittedIntegrator::integrate (Src/integrator.h:303-393) for one camera ray
template <typename TR>
__device__ v3 whit_integrate(const KParams& P, const TR& T, v3 ro, v3 rd, WhitCount& C) {
    const v3 sky = mk((float)0.235294, (float)0.67451, (float)0.843137);
    WRay q[kWhitQueue];
    uint32_t head = 0, tail = 0;
    v3 total = mk(0, 0, 0);
    q[0] = WRay{ro, rd, mk(1, 1, 1), 0u};
    tail = 1;
    while (head != tail) {
        const WRay ray = q[head & (kWhitQueue - 1u)];
        ++head;
        ++C.rays;
        if (ray.depth > P.max_depth) {
            total = total + ray.thr * sky;
            ++C.cut;
            continue;
        }
        HitRec h;
        T.closest(ray.o, ray.d, h);
        ++C.seg;
        Surf S;
        const int obj = T.surface(ray.o, ray.d, h, S);
        if (obj < 0) {
            total = total + ray.thr * sky;
            continue;
        }
        const int mat = T.obj[obj].material;
        if (mat == XRT_MAT_LAMBERT) {
            v3 rad = mk(0, 0, 0);
            const v3 fr = eval_bxdf(T.obj[obj]);
            for (int l = 0; l < P.n_dlights; ++l) {
                const DDelta& dl = P.dlights[l];
                v3 wi;
                float pdf, tmax;
                if (dl.kind == XRT_DLIGHT_POINT) {   // PointLight::sample (Src/light.cpp:120-128)
                    const v3 ld = ld3(dl.pos) - S.pos;
                    const float dist = length(ld);
                    wi = ld / dist;
                    pdf = dist * dist;
                    tmax = dist;
                } else {   // DistantLight::sample (Src/light.cpp:136-142)
                    wi = -ld3(dl.dir);
                    pdf = 1.0f;
                    tmax = kINF;
                }
                const bool vis = !T.occluded(S.pos + S.ng * 0.1f, wi, tmax);
                ++C.shadow;
                rad = rad + (((fr * (float)vis) * ld3(dl.L)) * smax(0.0f, dot(S.ns, wi))) / pdf;
            }
            rad = rad * ray.thr;
            total = total + rad;
        } else if (mat == XRT_MAT_METAL) {
            q[tail & (kWhitQueue - 1u)] =
                WRay{S.pos + S.ng * 0.001f, whit_reflect(ray.d, S.ng), ray.thr * 0.8f, ray.depth + 1u};
            ++tail;
        } else if (mat == XRT_MAT_GLASS) {
            const float kr = whit_fresnel(ray.d, S.ng, kWhitIor);
            const bool outside = dot(ray.d, S.ng) < 0.0f;
            const v3 bias = S.ng * 0.001f;
            const v3 thr9 = ray.thr * 0.9f;
            if (kr < 1.0f) {
                q[tail & (kWhitQueue - 1u)] = WRay{outside ? S.pos - bias : S.pos + bias,
                                                   normalize(whit_refract(ray.d, S.ng, kWhitIor)), thr9 * (1.0f - kr),
                                                   ray.depth + 1u};
                ++tail;
                ++C.refr;
            } else {
                ++C.tir;
            }
            q[tail & (kWhitQueue - 1u)] = WRay{outside ? S.pos + bias : S.pos - bias, normalize(whit_reflect(ray.d, S.ng)),
                                               thr9 * kr, ray.depth + 1u};
            ++tail;
        }
        // MaterialType::Unknow (no material: emitters, medium boxes): no contribution, no children
    }
    return total;
}

// One wave's share of the shard: pixels from the counter at `work` until it runs out, the
// pixel's stream in the wave's LDS slice st (kMT words, then the ordered-sum buffer), the
// samples' ray trees through the trace policy T.  Both kernels below are this loop.
// MOM (a variance render, xrt_render_var): the accepted samples' luminance l and l * l go through
// the same ordered sum, after the window's radiances, into two more running sums — lane 0 holds s1,
// lane 1 s2 — and the pixel's record mom[s] = {s1, s2} is written for k_finish_var (frame.hip).
template <bool MOM, typename TR>
__device__ __forceinline__ void whit_pixels(const KParams& P, const TR& T, uint32_t* st, uint32_t* __restrict__ work,
                                            int lane, float2* mom) {
    float* sum = reinterpret_cast<float*>(st + kMT);
    unsigned long long w_rays = 0, w_cut = 0, w_refr = 0, w_tir = 0;   // lane totals over this wave's pixels
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
        float* px = P.fb + 3 * ((size_t)col + (size_t)P.width * row);
        float acc = lane < 3 ? px[lane] : 0.0f;   // lane c < 3: channel c of the running sum
        uint32_t g = kMT;                         // x[0 .. g) generated; sample k draws x[kMT + 2k], x[kMT + 2k + 1]
        uint32_t nrej = 0;
        float macc = 0.0f;                        // MOM: lane 0 the running s1, lane 1 the running s2
        WhitCount C;
        for (uint32_t k0 = 0; k0 < P.spp; k0 += 64u) {
            const uint32_t span = min(64u, P.spp - k0);
            const uint32_t o = kMT + 2u * k0;
            while (g < o + 2u * span) {   // one chunk per window: g = o before it, o + 128 after
                pix_gen(st, g, lane);
                g += kPixChunk;
            }
            const bool act = (uint32_t)lane < span;
            v3 r = mk(0, 0, 0);
            if (act) {
                uint32_t ci = (o % kMT) + 2u * (uint32_t)lane;
                if (ci >= kMT) ci -= kMT;
                LdsRng rng{st, ci};
                const float jx = rng.next();
                const float jy = rng.next();
                v3 ro, rd;
                jitter_ray(P, col, row, jx, jy, ro, rd);
                r = whit_integrate(P, T, ro, rd, C) / 1.0f;
            }
            const uint64_t vm = __ballot(act && !radiance_invalid(r));
            nrej += span - (uint32_t)__builtin_popcountll(vm);
            pix_add_in_order(sum, lane, acc, vm, r);
            if (MOM) {
                const float l = luminance(r);
                pix_add_in_order(sum, lane, macc, vm, mk(l, l * l, 0.0f));
            }
        }
        if (lane < 3) px[lane] = acc;
        if (MOM && lane < 2) reinterpret_cast<float*>(mom + s)[lane] = macc;
        // the pixel's counters, as the per-slot schedules leave them for k_finish: its
        // Scene::intersect and Scene::occluded calls, its rejects, the stream cursor (two words
        // per sample) and the twists a std::mt19937 makes to produce that many words
        uint32_t nseg = C.seg, nsh = C.shadow;
        for (int off = 32; off > 0; off >>= 1) nseg += __shfl_down(nseg, off), nsh += __shfl_down(nsh, off);
        w_rays += C.rays, w_cut += C.cut, w_refr += C.refr, w_tir += C.tir;
        if (lane == 0) {
            const uint32_t o = kMT + 2u * P.spp;
            P.c_seg[s] = nseg;
            P.c_shadow[s] = nsh;
            P.c_rej[s] = nrej;
            P.c_stall[s] = 0;
            P.rng_c[s] = o;
            P.rng_g[s] = kMT + kMT * ((o - kMT + kMT - 1u) / kMT);
            P.sample_k[s] = P.spp;
            P.state[s] = ST_DONE;
        }
        wave_sync();   // the stream buffer is reloaded for the next pixel
    }
    const unsigned long long c[4] = {w_rays, w_cut, w_refr, w_tir};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned long long v = c[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0 && v) atomicAdd(P.stats + kStatsWhit + q, v);
    }
}

template <int SCN, bool MOM = false>
__global__ __launch_bounds__(kWhitBlock) void k_whitted(KParams P, uint32_t* __restrict__ work, float2* mom) {
    extern __shared__ __attribute__((aligned(16))) f4 lds_whit[];
    char* lb = reinterpret_cast<char*>(lds_whit);
    const int tid = threadIdx.x, lane = tid & 63;
    const LScene L = load_lscene(P, lb, tid, kWhitBlock);
    uint32_t* st = reinterpret_cast<uint32_t*>(lb + whit_wave_off(P) + (tid >> 6) * kWhitWaveLds);
    __syncthreads();
    const WhitLds<SCN> T{P, L, L.obj};
    whit_pixels<MOM>(P, T, st, work, lane, mom);
}

// ------------------------------------------------------------ scenes beyond LDS ----
// k_whitted_bvh: the same wave-per-pixel loop for triangle scenes that do not fit the LDS
// scene carve but have the triangle BVH xrt_upload_scene builds (bvh.h): every triangle in
// it (one-level scenes), or the large meshes in it and the small objects beside it (two-level
// scenes, C4).  Only the three scene accessors differ from k_whitted:
//
//   closest   Scene::intersect's result is the lexicographic minimum of (t, original triangle
//             index) over all triangles (the in-order strict `t < best` scan).  Two-level: the
//             small objects first, from their LDS copy, in object order with k_trace_2a's
//             plane and box culls and its strict `t < best` — the (t, index) minimum among
//             them, their triangles being in index order — carrying the original index
//             (e2.w); then, if the segment [0, best t] reaches the BVH root (inclusive: an
//             equal t with a lower index must still be found), bvh_trace starts from that hit
//             and bvh_leaf's `t < bt || (t == bt && k < bk)` merges the large meshes' triangles
//             into it: the minimum over both sets, what k_trace_2a + k_trace_deep4 compute.
//             One-level: bvh_trace alone, from a miss.  The culls are conservative (padded
//             boxes, the plane argument of DESIGN.md §3), so they never drop a hit the scan
//             accepts.
//   occluded  Scene::occluded: the small objects that occlude (count_occ's sign bit: no area
//             light) first, then bvh_trace<true>, which skips area-light triangles (B.w == 0).
//   surface   surface<SCN_TRI> (path_common.h) over the global arrays: tri_ng, tri_nrm, the
//             object index in tri[3 * idx].w; material and albedo from the global object table.
//
// Rays arrive as Whitted makes them.  A metal child's direction is not normalised: the slab
// tests and Moller-Trumbore are consistent under a scale of d (t scales with it).  A NaN
// direction (normalize of refract's zero vector) must miss everything, and does: its
// reciprocal is NaN, fminf / fmaxf drop the NaNs so box_overlap and bvh_enter enter every box,
// plane_away_w's comparison is false, and every ray_tri fails its final `t > eps` — the walk
// visits the whole tree once and ends as a miss.  Zero-edge triangles of the large meshes
// are not in the BVH (xrt_upload_scene) and no ray_tri accepts them anyway.
// The traversal stack (P.bvh_stack entries per thread, 16-bit when the node indices fit) and
// the top of the tree are in LDS as in k_trace_bvh; the ray ring stays in scratch.  The layout
// and the policy (WhitBvhLayout, WhitBvh) are in whit_trace.h.
template <bool TWO, typename SE, bool MOM = false>
__global__ __launch_bounds__(kWhitBlock) void k_whitted_bvh(KParams P, uint32_t* __restrict__ work, float2* mom) {
    extern __shared__ __attribute__((aligned(16))) f4 lds_whit_bvh[];
    const auto B = whit_bvh_setup<TWO, SE>(P, reinterpret_cast<char*>(lds_whit_bvh), threadIdx.x);
    whit_pixels<MOM>(P, B.T, B.st, work, threadIdx.x & 63, mom);
}

// device self-test (xrt_test_whitted_math): the kernel's own geometry functions
__global__ __launch_bounds__(kBlock) void k_test_whitted(const float* in, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const v3 I = ld3(in + 6 * (size_t)i), N = ld3(in + 6 * (size_t)i + 3);
    const v3 rl = whit_reflect(I, N), rr = whit_refract(I, N, kWhitIor);
    const v3 nl = normalize(rl), nr = normalize(rr);
    float* o = out + 13 * (size_t)i;
    o[0] = rl.x, o[1] = rl.y, o[2] = rl.z, o[3] = rr.x, o[4] = rr.y, o[5] = rr.z;
    o[6] = whit_fresnel(I, N, kWhitIor);
    o[7] = nl.x, o[8] = nl.y, o[9] = nl.z, o[10] = nr.x, o[11] = nr.y, o[12] = nr.z;
}

}  // namespace xrt

#include "launch.h"

namespace xrt {

size_t whit_lds_bytes(const KParams& P) { return whit_wave_off(P) + (size_t)(kWhitBlock / 64) * kWhitWaveLds; }

bool use_whitted(const KParams& P) {
    // the scene fits the LDS carve (not a two-level scene) and, with the waves' slices, what
    // this device gives a workgroup
    return step_lds_bytes(P) != 0 && !P.two_level && whit_lds_bytes(P) <= kPixLds && whit_lds_bytes(P) <= P.lds_max;
}

// one launch of a Whitted kernel over the shard's pixels: a persistent grid, at most one wave per pixel
template <typename K>
static hipError_t whit_launch(K kern, size_t lds, const KParams& P, uint32_t* work, hipStream_t st, float2* mom) {
    uint32_t blocks = 0;
    const hipError_t e = persistent_blocks(kern, kWhitBlock, lds, P.n_slots, &blocks);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWhitBlock), lds, st, P, work, mom);
    return hipGetLastError();
}

hipError_t launch_whitted(const KParams& P, uint32_t* work, hipStream_t st, float2* mom) {
    if (!use_whitted(P)) return hipErrorInvalidValue;
    if (hipMemsetAsync(work, 0, sizeof(uint32_t), st) != hipSuccess) return hipErrorInvalidValue;
    return with_scene_kind(P.scene_kind, [&](auto scn) {
        return with_const<1, 0>(mom != nullptr, [&](auto m) {
            return whit_launch(k_whitted<decltype(scn)::value, decltype(m)::value != 0>, whit_lds_bytes(P), P, work, st, mom);
        });
    });
}

size_t whit_bvh_lds_bytes(const KParams& P) { return whit_bvh_layout(P).total; }

bool use_whitted_bvh(const KParams& P) {
    // a triangle scene with the BVH over its (large meshes') triangles, a tree the stack was
    // sized for, small objects within the LDS scan's bounds, and an LDS sum this device gives
    return P.scene_kind == SCN_TRI && P.bvh_node && P.bvh_tri && P.bvh_nodes > 0 && P.bvh_stack > 0 &&
           P.bvh_stack <= kBvhStack &&
           (!P.two_level || (P.stri && P.sbox && P.splane && P.n_stri <= kSmallTris && P.n_sobj <= kSmallObjs)) &&
           whit_bvh_lds_bytes(P) <= kPixLds && whit_bvh_lds_bytes(P) <= P.lds_max;
}

hipError_t launch_whitted_bvh(const KParams& P, uint32_t* work, hipStream_t st, float2* mom) {
    if (!use_whitted_bvh(P)) return hipErrorInvalidValue;
    if (hipMemsetAsync(work, 0, sizeof(uint32_t), st) != hipSuccess) return hipErrorInvalidValue;
    return with_whit_bvh(P, [&](auto two, auto se) {
        return with_const<1, 0>(mom != nullptr, [&](auto m) {
            return whit_launch(k_whitted_bvh<decltype(two)::value, decltype(se), decltype(m)::value != 0>,
                               whit_bvh_lds_bytes(P), P, work, st, mom);
        });
    });
}

hipError_t launch_test_whitted(const float* in, uint32_t n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_test_whitted, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, in, n, out);
    return hipGetLastError();
}

}  // namespace xrt
