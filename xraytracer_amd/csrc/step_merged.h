// step_merged.h — merged-trace fused schedule for small triangle scenes (C1, C2: the
// Cornell box), the latency-critical kernel of the renderer: the body, its three kernels and their
// launch dispatch, as templates.  step_merged.hip instantiates the plain builds, step_merged_mom.hip
// the moments builds (MOM): as many instantiations of the body again, compiled beside the first
// unit instead of after it.
//
// Same per-pixel sequence as NormalRenderer::doRender + GIIntegrator / DirectIntegrator
// (Src/renderer.cpp:29-81, Src/integrator.h:82-119, 205-287), one path slot per pixel, path
// state in registers for `visits` segments per launch.  What differs from k_step_tri
// (step.hip) is the schedule of the traces:
//
//  * One cooperative trace per segment.  The NEE shadow rays of segment i and the
//    extension ray of segment i+1 (or the next sample's camera ray) are traced together:
//    every RNG draw of segment i (RR, light samples, BSDF sample, the next sample's jitter)
//    happens in the reference's order before either ray is traced, and the occlusion
//    result only changes the radiance, never a draw.  The contribution is kept for both
//    outcomes (c1: visible, c0: occluded — the reference multiplies by vis first, so both
//    are computed with its operation order) and added after the trace, still before any
//    later radiance update of the same path, so every float sum happens in the
//    reference's order.  A sample that ends with shadow rays in flight is finished after
//    they resolve (rad_fin), while its successor's camera ray is traced.
//  * Class-major pair passes (merged_trace, merged.h): for each object (kernel-argument record,
//    scalar loads) the
//    wave ballots which of its rays (1 + NL per lane) overlap the object's culling box and
//    ranks those rays into LDS (mbcnt; origin + tmax, direction + the object's first triangle
//    and the ray id), the objects of one triangle count (a class, StepClass) one behind the
//    other in one stream; then it tests the class's (ray, triangle) pairs 64 per pass,
//    pair j -> ray rank j / count (magic multiply), triangle first(ray) + j % count.  No prefix
//    scan, no per-lane expansion loop, no per-pair table: the count is uniform within the
//    stream.  Closest hits merge with an LDS atomicMin of
//    (t bits << 32 | triangle): smallest t, ties to the lower triangle index — the
//    reference's in-order strict `t < best` scan; shadow rays set an occlusion bit.
//  * The RNG words a segment can use (6 + 2 NL at most) are prefetched into registers by
//    global (not flat) loads issued one segment ahead.
//
// GIIntegrator with maxDepth 0 and scenes with more than kMergedMaxObjs objects keep using
// k_step_tri.
#pragma once
#include <type_traits>

#include "launch.h"
#include "merged.h"
#include "path_common.h"
#include "step_sources.h"
#include "wave_deep.h"

namespace xrt {

// Experiment builds (XRT_PHASE_CLOCK, tools/wave_timeline.py): lane 0 of every wave of the merged
// kernels records the constant-rate wall clock and the shader clock at entry and at exit, one
// record per wave in launch order of arrival; render_impl writes the records of a render to the
// file XRT_WAVE_CLOCK_OUT names (wave_clock_dump, step_merged.hip).  tag: the launch's group
// argument, ~0 ungrouped.  The moments builds record no clocks: the buffer is the plain unit's.
struct NoWaveClock {
    __device__ explicit NoWaveClock(uint32_t) {}
    __device__ void end() {}
};
#if XRT_PHASE_CLOCK
constexpr uint32_t kWaveClockCap = 1u << 20;
struct WaveClockRec {
    uint32_t tag, block;
    unsigned long long wall0, shader0, wall1, shader1;
};
static __device__ WaveClockRec g_wave_clock[kWaveClockCap];
static __device__ unsigned int g_wave_clock_n;
struct WaveClock {
    uint32_t idx = kWaveClockCap;
    __device__ explicit WaveClock(uint32_t tag) {
        if ((threadIdx.x & 63u) == 0u) {
            idx = atomicAdd(&g_wave_clock_n, 1u);
            if (idx < kWaveClockCap) {
                g_wave_clock[idx].tag = tag, g_wave_clock[idx].block = blockIdx.x;
                g_wave_clock[idx].wall0 = wall_clock64(), g_wave_clock[idx].shader0 = clock64();
            }
        }
    }
    __device__ void end() {
        if (idx < kWaveClockCap) g_wave_clock[idx].wall1 = wall_clock64(), g_wave_clock[idx].shader1 = clock64();
    }
};
#else
using WaveClock = NoWaveClock;
#endif

// SPW: path slots per wave (64, 32 or 16), G: lanes per slot (1, or 64 / SPW for the group
// trace).  With G = 1 and SPW < 64, lanes >= SPW own no slot but take part in every pair
// pass of the cooperative traces, so a half- or quarter-filled wave traces its rays in
// proportionally fewer passes; with G > 1 every lane of a slot's group runs its path
// (redundantly, results identical) and the group shares the traces (group_trace).  Either
// way, with few slots per GPU (a pixel shard of a multi-GPU frame) this puts more, shorter
// waves on every SIMD.
// BVH: two-level scenes (use_step_bvh: C4) — the small objects' triangles in LDS and traced
// by merged_trace with original-index keys, the rest by the wave's BVH walk (deep_pass, wave_deep.h);
// the hit triangle's shading data from global memory.  Same path
// code otherwise.
//
// src: the launch's slot source (step_sources.h) — every partition, one partition group, or the
// block's own chunks.  The body is one loop over its passes; nothing inside a visit depends on it.
// visits_arg: the visits per pass as the source reads them (src.visits: the chunk kernel packs its
// passes above them).
//
// MOM (a variance render under XRT_FLAG_VAR_FUSED, xrt_render_var): an accepted sample also adds its
// luminance l and l * l to the slot's record mom[s] = {s1, s2} (k_finish_var, frame.hip, turns the
// records into the plane); mom is null otherwise.  Every sample end passes through `finish` — the direct end, the
// deferred one (fin / rad_fin) and the drain — so that is the one site.  The record is carried in
// registers for the launch, loaded and stored beside the pixel's sum: every lane of a slot's group
// carries the same bits and the lead lane stores (XRT_MOM_REGS, tuning.h; 0: a read-modify-write at
// the site by the lead lane, measured 2-5 % slower).  The records are zeroed before
// seeding (render_impl): k_camlist's retired pixels never reach this kernel.
template <int INTEG, int NL, int SPW, int G, bool LANE, bool BVH, bool MOM, typename SRC>
__device__ __forceinline__ void step_merged_body(
    const KParams* __restrict__ Pp, const StepObjs SO,   // by value as the kernels take it (by reference: 4 spilled VGPRs in the group kernel for 2)
    const SRC src, float2* mom, const uint32_t visits_arg) {
    constexpr int NW = 6 + 2 * NL;   // most words one segment draws (see the header)
    static_assert(SRC::template layout_ok<SPW, G, LANE, BVH, MOM>(), "the slot source does not serve this layout");
    std::conditional_t<MOM, NoWaveClock, WaveClock> wclk(src.clock_tag());   // experiment builds (XRT_PHASE_CLOCK): the wave's entry and exit clocks
    static_assert(!BVH || (G == 1 && !LANE), "two-level scenes trace by pair passes");
    const KParams& P = *Pp;
    extern __shared__ __attribute__((aligned(16))) f4 lds_m[];
    char* lb = reinterpret_cast<char*>(lds_m);
    const int tid = threadIdx.x, lane = tid & 63;
    LScene L;
    const DObjPlane* lplane = nullptr;
    MergedWave<NL>* Wp;
    const f4* top = nullptr;   // BVH: the first ntop 4-wide nodes
    uint16_t* stk = nullptr;   // BVH: this wave's quad stacks
    int ntop = 0;
    f4 root[4];                // BVH: the binary root node (deep_pass's root test)
    if constexpr (BVH) {
        const BvhStepLayout Bl = bvh_step_layout(P, (uint32_t)sizeof(MergedWave<NL>));
        L.tri = reinterpret_cast<const f4*>(lb + Bl.tri);
        L.obj = reinterpret_cast<const DObj*>(lb + Bl.obj);
        L.light = reinterpret_cast<const DLight*>(lb + Bl.light);
        top = reinterpret_cast<const f4*>(lb + Bl.top);
        ntop = Bl.ntop;
        Wp = reinterpret_cast<MergedWave<NL>*>(lb + Bl.wave);
        stk = reinterpret_cast<uint16_t*>(lb + Bl.stack + (tid >> 6) * kStackWave);
        lds_copy(const_cast<f4*>(L.tri), P.stri, 3 * P.n_stri, tid);
        lds_copy(const_cast<DObj*>(L.obj), P.objs, P.n_objs, tid);
        lds_copy(const_cast<DLight*>(L.light), P.lights, P.n_lights, tid);
        lds_copy(const_cast<f4*>(top), P.bvh4, 8 * ntop, tid);
        root[0] = ldg4(P.bvh_node, 0), root[1] = ldg4(P.bvh_node, 1), root[2] = ldg4(P.bvh_node, 2);
        root[3] = ldg4(P.bvh_node, 3);
    } else {
        const StepLayout Lo = step_layout(P);
        L.tri = reinterpret_cast<const f4*>(lb + Lo.tri);
        L.tng = reinterpret_cast<const f4*>(lb + Lo.tng);
        L.nrm = reinterpret_cast<const f4*>(lb + Lo.nrm);
        L.box = reinterpret_cast<const DObjBox*>(lb + Lo.box);
        L.sph = reinterpret_cast<const f4*>(lb + Lo.sph);
        L.bx = reinterpret_cast<const f4*>(lb + Lo.bx);
        L.obj = reinterpret_cast<const DObj*>(lb + Lo.obj);
        L.light = reinterpret_cast<const DLight*>(lb + Lo.light);
        L.sobj = reinterpret_cast<const int*>(lb + Lo.sobj);
        lplane = reinterpret_cast<const DObjPlane*>(lb + merged_plane_off(Lo));
        Wp = reinterpret_cast<MergedWave<NL>*>(lb + merged_wave_off(P, Lo));
        lds_copy(const_cast<f4*>(L.tri), P.tri, 3 * P.n_tris, tid);
        lds_copy(const_cast<f4*>(L.tng), P.tri_ng, P.n_tris, tid);
        lds_copy(const_cast<f4*>(L.nrm), P.tri_nrm, 3 * P.n_tris, tid);
        lds_copy(const_cast<DObj*>(L.obj), P.objs, P.n_objs, tid);
        lds_copy(const_cast<DLight*>(L.light), P.lights, P.n_lights, tid);
        if (LANE) {
            lds_copy(const_cast<DObjBox*>(L.box), P.obj_box, P.n_objs, tid);
            lds_copy(const_cast<DObjPlane*>(lplane), P.obj_plane, P.n_objs, tid);
        }
    }
    MergedWave<NL>& W = Wp[tid >> 6];
    static_assert(sizeof(MergedWave<NL>) >= kMT * 4, "the wave's trace scratch doubles as the refill buffer");
    // the hit triangle's records: LDS (the whole scene is there) or, two-level, global memory
    // (hk is then the triangle's original index)
    auto tri_rec = [&](int i) -> f4 {
        if constexpr (BVH) return ldg4(P.tri, i);
        else return L.tri[i];
    };
    auto tri_ng_at = [&](int i) -> v3 {
        if constexpr (BVH) return xyz(ldg4(P.tri_ng, i));
        else return xyz(L.tng[i]);
    };
    auto tri_ns_at = [&](int i, float u, float v) -> v3 {
        if constexpr (BVH) {
            const float w = 1.0f - u - v;
            return xyz(ldg4(P.tri_nrm, 3 * (size_t)i)) * w + xyz(ldg4(P.tri_nrm, 3 * (size_t)i + 1)) * u +
                   xyz(ldg4(P.tri_nrm, 3 * (size_t)i + 2)) * v;
        } else {
            return tri_ns_l(L, i, u, v);
        }
    };
    __syncthreads();
    // the next-next round's counters this launch owns.  The request counter is not
    // touched here (only the seeding refill reads a request list)
    src.clear(P);
    auto ps = src.begin(P, (kBlock / 64) * SPW, visits_arg);   // the block's place in its lists
    const uint32_t visits = src.visits(visits_arg);
    const uint32_t spp = P.spp, max_depth = P.max_depth, width = P.width;
    for (uint32_t base = src.first(ps); src.next_pass(ps, base); base += src.stride(ps)) {
        const uint32_t n_in = src.n_in(ps);   // entries of the list this pass reads
        const uint32_t i = base + (uint32_t)(tid >> 6) * SPW + (uint32_t)lane / G;
        const bool own = lane / G < SPW && i < n_in;
        const bool lead = own && (lane % G) == 0;   // the lane of a group that writes back
        const uint32_t s = own ? src.slot(P, ps, i) : 0;
        uint32_t st = own ? glb<gu32>(P.state)[s] : ST_DONE;
        st &= ~ST_RNGREQ;   // the refill this slot asked for ran after the previous launch
        const bool live = !(st & ST_DONE);
        uint32_t g = 0, depth = 0, k = 0, kst = 0;   // k: finished samples, kst: started samples
        RngRegs<NW> rng;
        rng.c = 0;
        const uint32_t* ring = P.ring + (size_t)s * kRing;
        v3 thr = mk(1, 1, 1), rad = mk(0, 0, 0), o = mk(0, 0, 0), d = mk(0, 0, 0), acc = mk(0, 0, 0);
        v3 rad_fin = mk(0, 0, 0), thr_nee = mk(0, 0, 0);
        v3 so[NL + 1], sd[NL + 1], c1[NL + 1], c0[NL + 1];
        // GI with one light: the NEE term is folded at sampling time — c1[0] holds
        // thr * (0 + (0 + c1)) and c0z the codes of thr * (0 + (0 + c0)) (each component +-0 or
        // NaN), the exact values resolve() would form from thr_nee and c0 / c1 — so neither
        // thr_nee nor c0 stays live across the trace
        constexpr bool kFold = INTEG == XRT_INTEGRATOR_GI && NL == 1;
        // the state word's covering triangle is set only where k_camlist retires (plan_render's elide)
        constexpr bool kCover = XRT_CAM_COVER && INTEG == XRT_INTEGRATOR_GI && !BVH;
        uint32_t c0z = 0;
        float stm[NL + 1];
#pragma unroll
        for (int l = 0; l <= NL; ++l) so[l] = sd[l] = c1[l] = c0[l] = mk(0, 0, 0), stm[l] = 0.0f;
        uint32_t shm = 0;          // shadow rays in flight (bit per light)
        bool ext = false, fin = false;
        float2 msum = make_float2(0.0f, 0.0f);   // MOM with XRT_MOM_REGS: the slot's record, carried like acc
        const SlotPixel pix = slot_pixel(P, s);
        const uint32_t col = pix.col, row = pix.row;
        float* px = P.fb + 3 * ((size_t)col + (size_t)width * row);
        if (live) {
            g = glb<gu32>(P.rng_g)[s];
            rng.c = glb<gu32>(P.rng_c)[s];
            depth = glb<gu32>(P.depth)[s];
            k = glb<gu32>(P.sample_k)[s];
            kst = k;
            if (!(st & ST_REGEN)) {
                thr = ld3g(P.thr, s), rad = ld3g(P.rad, s);
                o = ld3g(P.ray_o, s), d = ld3g(P.ray_d, s);
                ext = true;
                kst = k + 1;
            }
            gf32* pxg = glb<gf32>(px);
            acc = mk(pxg[0], pxg[1], pxg[2]);
            if constexpr (MOM && XRT_MOM_REGS) msum = mom[s];
            rng.load(ring);
        }
        uint32_t nseg = 0, nsh = 0, nrej = 0;
        // Image::addPixel of a finished sample (Src/renderer.cpp:57-75)
        auto finish = [&](v3 r0) {
            const v3 r = r0 / 1.0f;
            // radiance_invalid (path_common.h), open-coded: the call changes this kernel's instructions
            if (__builtin_isnan(r.x) || __builtin_isnan(r.y) || __builtin_isnan(r.z) || __builtin_isinf(r.x) ||
                __builtin_isinf(r.y) || __builtin_isinf(r.z) || r.x < 0.0f || r.y < 0.0f || r.z < 0.0f) {
                ++nrej;
            } else {
                acc = acc + r;
                if constexpr (MOM) {   // s1 = s1 + l, s2 = s2 + l * l (include/xrt.h, xrt_render_var)
                    const float l = luminance(r);
                    if constexpr (XRT_MOM_REGS) {   // every lane of a group carries the same bits
                        msum.x = msum.x + l, msum.y = msum.y + l * l;
                    } else if (lead) {
                        float2 m = mom[s];
                        m.x = m.x + l, m.y = m.y + l * l;
                        mom[s] = m;
                    }
                }
            }
            ++k;
            if (k >= spp) st = ST_DONE;
        };
        // jitter draws + PinholeCamera::sampleRay for the next sample (Src/renderer.cpp:44-50)
        auto start_sample = [&]() {
            // sample_start (path_common.h), open-coded: the call changes this kernel's instructions
            const float u = div_w(P, (float)(int)col + rng.next());
            const float v = div_h(P, (float)(int)row + rng.next());
            camera_ray(P, u, v, o, d);
            thr = mk(1, 1, 1), rad = mk(0, 0, 0);
            depth = 0;
            ext = true;
            ++kst;
        };
        // add the resolved NEE of the last shaded segment (GI: rad += thr * directL;
        // Direct: L += L_light per light) and finish its sample if it ended there
        auto resolve = [&](uint32_t occ) {
            if (!shm) return;
            v3& tgt = fin ? rad_fin : rad;
            if (INTEG == XRT_INTEGRATOR_DIRECT) {
#pragma unroll
                for (int l = 0; l < NL; ++l)
                    if ((shm >> l) & 1u) tgt = tgt + (((occ >> l) & 1u) ? c0[l] : c1[l]);
            } else if constexpr (kFold) {
                tgt = tgt + ((occ & 1u) ? mk(zdecode(c0z & 3u), zdecode((c0z >> 2) & 3u), zdecode(c0z >> 4)) : c1[0]);
            } else {
                v3 directL = mk(0, 0, 0);
#pragma unroll
                for (int l = 0; l < NL; ++l)
                    if ((shm >> l) & 1u) {
                        const v3 L_light = mk(0, 0, 0) + (((occ >> l) & 1u) ? c0[l] : c1[l]);
                        directL = directL + L_light;
                    }
                tgt = tgt + thr_nee * directL;
            }
            shm = 0;
            if (fin) {
                fin = false;
                finish(rad_fin);
            }
        };
        // a slot that starts a sample at the launch's first segment draws its jitter from
        // the words loaded above; later segments start samples at their end (start_sample
        // below), so no draw precedes the trace inside the loop
        if (live && !(st & ST_DONE) && g - rng.c >= (uint32_t)NW && (st & ST_REGEN)) {
            st &= ~ST_REGEN;
            start_sample();
        }
        __builtin_amdgcn_s_waitcnt(0);   // prologue loads done: the loop waits only on its own prefetches
        bool pf_pending = false;   // BVH: words in pf[]
        for (uint32_t vis = 0; vis < visits; ++vis) {
            const bool act = live && !(st & ST_DONE) && g - rng.c >= (uint32_t)NW;
            if (!__ballot(act || shm)) break;
            const bool ext_now = act && ext;
            // a camera ray of a pixel that one triangle covers (k_camlist's covering claim, the
            // triangle + 1 in the state word) hits that triangle first, whatever its jitter: it is
            // not traced, and the shading below recomputes t, u, v from the triangle as for any hit
            const bool ext_tr = ext_now && !(kCover && depth == 0 && (st >> ST_COVER_SHIFT));
            unsigned long long best;
            uint32_t occ;
            if constexpr (BVH) {
                merged_trace<NL, true>(SO, L, W, lane, ext_now, o, d, shm, so, sd, stm, best, occ);
                deep_pass<NL, uint16_t>(P, top, ntop, stk, W, lane, root, ext_now, o, d, shm, so, sd, stm, best, occ);
            } else if constexpr (!LANE) {
                merged_trace<NL>(SO, L, W, lane, ext_tr, o, d, shm, so, sd, stm, best, occ);
            } else {
                group_trace<NL, G>(P.n_objs, L, lplane, lane, ext_tr, o, d, shm, so, sd, stm, best, occ);
            }
            if (kCover && ext_now && depth == 0 && (st >> ST_COVER_SHIFT)) best = (st >> ST_COVER_SHIFT) - 1u;
            resolve(occ);
            if (BVH ? pf_pending : vis > 0) rng.take();   // the words prefetched at the end of the previous segment
            if (ext_now) {
                ++nseg;
                int hk = -1, obj = -1;
                float ht = kINF, hu = 0.0f, hv = 0.0f;
                if (best != ~0ull) {
                    hk = (int)(uint32_t)best;
                    const f4 ta = tri_rec(3 * hk);
                    (void)ray_tri(o, d, xyz(ta), xyz(tri_rec(3 * hk + 1)), xyz(tri_rec(3 * hk + 2)), ht, hu, hv);
                    obj = __float_as_int(ta.w);
                }
                v3 pos = mk(0, 0, 0), ng = mk(0, 0, 0);
                if (hk >= 0) pos = ray_at(o, d, ht), ng = tri_ng_at(hk);
                bool ended = false, alive = false;
                if (INTEG == XRT_INTEGRATOR_DIRECT) {
                    // DirectIntegrator::integrate (Src/integrator.h:82-119)
                    if (obj < 0) {
                        rad = mk((float)0.18, (float)0.18, (float)0.18);
                        ended = true;
                    } else if (L.obj[obj].light >= 0) {
                        rad = light_Le(L.light[L.obj[obj].light], tri_ns_at(hk, hu, hv), d);
                        ended = true;
                    } else {
                        alive = true;
                    }
                } else {
                    // GIIntegrator::integrate loop body (Src/integrator.h:214-284)
                    if (obj < 0) {
                        rad = rad + thr * mk(0.0f, 0.0f, 0.0f);
                        ended = true;
                    } else {
                        alive = true;
                        if (depth > 0) {
                            const float pr = smin(div_const(thr.x + thr.y + thr.z, 3.0f, kRcp3), 1.0f);
                            if (rng.next() >= pr) alive = false, ended = true;
                            else thr = thr / mk(pr, pr, pr);
                        }
                        if (alive && L.obj[obj].light >= 0) {
                            if (depth == 0)
                                rad = rad + thr * light_Le(L.light[L.obj[obj].light], tri_ns_at(hk, hu, hv), d);
                            alive = false, ended = true;
                        }
                    }
                }
                if (alive) {
                    // next-event estimation: light samples now, shadow rays traced with the
                    // next trace of the wave
                    const DObj& ob = L.obj[obj];
                    const v3 fr = ob.material == 1 ? mk(ob.fr[0], ob.fr[1], ob.fr[2]) : mk(0, 0, 0);
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        v3 wi = mk(0, 0, 0);
                        float tmax = 0.0f, pdf = 0.0f;
                        const v3 Lv = light_sample(L.light[l], pos, wi, pdf, tmax, rng);
                        if (pdf != 0.0f) {
                            ++nsh;
                            shm |= 1u << l;
                            const float bias = 0.01f;
                            so[l] = pos + ng * bias, sd[l] = wi, stm[l] = tmax - bias;
                            const float cosv = smax(0.0f, dot(ng, wi));
                            // vis * fr * L * cos / pdf (Src/integrator.h:250-262) for vis = 1, 0.
                            // fr * 1 == fr; for vis = 0 the product is +-0 or NaN and pdf is
                            // > 0 (or NaN), so the quotient is that product (NaN for a NaN pdf)
                            c1[l] = ((fr * Lv) * cosv) / pdf;
                            const v3 z = ((fr * 0.0f) * Lv) * cosv;
                            c0[l] = pdf == pdf ? z : mk(pdf, pdf, pdf);
                            if constexpr (kFold) {   // GIIntegrator: rad += thr * directL (resolve)
                                const v3 zero = mk(0, 0, 0);
                                c1[0] = thr * (zero + (zero + c1[0]));
                                const v3 w = thr * (zero + (zero + c0[0]));
                                c0z = zcode(w.x) | (zcode(w.y) << 2) | (zcode(w.z) << 4);
                            }
                        }
                    }
                    if (INTEG == XRT_INTEGRATOR_DIRECT) {
                        ended = true;
                    } else {
                        if (!kFold && shm) thr_nee = thr;
                        else rad = rad + thr * mk(0.0f, 0.0f, 0.0f);   // no shadow ray: directL = 0
                        v3 nd = mk(0, 0, 0);
                        const bool lamb = ob.material == 1;
                        if (lamb) {
                            v3 dpdu, dpdv;
                            onb(tri_ns_at(hk, hu, hv), dpdu, dpdv);
                            nd = lambert_sample_f(ng, dpdu, dpdv, rng);
                        }
                        const float cosv = smax(0.0f, dot(nd, ng));
                        // (fr * cos) / pdf, pdf = 1 / (2 PI) for Lambert (Src/material.h:60-73), else 1
                        const v3 fc = fr * cosv;
                        thr = thr * (lamb ? mk(div_const(fc.x, kLambertPdf, kLambertPdfRcp),
                                               div_const(fc.y, kLambertPdf, kLambertPdfRcp),
                                               div_const(fc.z, kLambertPdf, kLambertPdfRcp))
                                          : fc / 1.0f);
                        o = pos + ng * 0.01f;
                        d = nd;
                        ++depth;
                        if (depth >= max_depth) ended = true;
                    }
                }
                if (ended) {
                    ext = false;
                    if (shm) {
                        rad_fin = rad;
                        fin = true;
                    } else {
                        finish(rad);
                    }
                    if (kst < spp) start_sample();
                }
            }
            rng.prefetch(ring);   // unconditional; first read by take() after the next trace
            pf_pending = true;
        }
        // drain: trace the shadow rays still in flight, so no NEE state crosses launches
        if (__ballot(shm != 0)) {
            unsigned long long best;
            uint32_t occ;
            if constexpr (BVH) {
                merged_trace<NL, true>(SO, L, W, lane, false, o, d, shm, so, sd, stm, best, occ);
                deep_pass<NL, uint16_t>(P, top, ntop, stk, W, lane, root, false, o, d, shm, so, sd, stm, best, occ);
            } else if constexpr (!LANE) {
                merged_trace<NL>(SO, L, W, lane, false, o, d, shm, so, sd, stm, best, occ);
            } else {
                group_trace<NL, G>(P.n_objs, L, lplane, lane, false, o, d, shm, so, sd, stm, best, occ);
            }
            resolve(occ);
        }
        bool want_req = false;
        if (live && lead) {
            px[0] = acc.x, px[1] = acc.y, px[2] = acc.z;
            if constexpr (MOM && XRT_MOM_REGS) mom[s] = msum;
            want_req = !(st & ST_DONE) && g - rng.c < P.rng_keep;
            P.state[s] = st;
            if (!(st & (ST_DONE | ST_REGEN))) {
                P.depth[s] = depth;
                P.thr[s] = pk(thr);
                P.rad[s] = pk(rad);
                P.ray_o[s] = pk(o);
                P.ray_d[s] = pk(d);
            }
            P.sample_k[s] = k;
            P.rng_c[s] = rng.c;
            if (nseg) P.c_seg[s] += nseg;
            if (nsh) P.c_shadow[s] += nsh;
            if (nrej) P.c_rej[s] += nrej;
        }
        src.append(P, ps, live && lead && !(st & ST_DONE), s, lane, tid);
        wave_refill(P, want_req, s, g, lane, reinterpret_cast<uint32_t*>(&W));
        src.pass_end();
    }
    if (tid == 0) src.finish(P, ps);
    wclk.end();
}

// The kernels' req_count argument: the request counter, which no step kernel reads (kept in the
// argument list of every schedule's step launch) — in a moments build the slots' records instead.
template <bool MOM>
using ReqOrMom = std::conditional_t<MOM, float2*, uint32_t*>;
template <bool MOM>
__device__ __forceinline__ float2* mom_of(ReqOrMom<MOM> req_count) {
    if constexpr (MOM) return req_count;
    else return nullptr;
}

// WV (two-level scenes): a register budget for WV waves per SIMD instead of XRT_BVH_WAVES, for
// launches with too few live slots to fill more (fewer spills)
template <int INTEG, int NL, int SPW, int G, bool LANE, bool BVH, int WV = 0, bool MOM = false>
__global__ __launch_bounds__(kBlock, WV ? WV : (BVH ? XRT_BVH_WAVES : XRT_STEP_WAVES)) void k_step_merged(
    const KParams* __restrict__ Pp, const StepObjs SO, const uint32_t* __restrict__ list,
    const uint32_t* __restrict__ count, uint32_t* __restrict__ out, uint32_t* out_count, uint32_t* zero_count,
    ReqOrMom<MOM> req_count, uint32_t visits) {
    step_merged_body<INTEG, NL, SPW, G, LANE, BVH, MOM>(Pp, SO, EveryPart{{list, count, out, out_count, zero_count}},
                                                        mom_of<MOM>(req_count), visits);
}

// The same kernel for one partition group of a round (whole waves of a one-level scene): the group
// as one trailing argument.  A kernel of its own, so that a launch of every partition stays the
// kernel it was, argument list included.
template <int INTEG, int NL, bool MOM = false>
__global__ __launch_bounds__(kBlock, XRT_STEP_WAVES) void k_step_merged_group(
    const KParams* __restrict__ Pp, const StepObjs SO, const uint32_t* __restrict__ list,
    const uint32_t* __restrict__ count, uint32_t* __restrict__ out, uint32_t* out_count, uint32_t* zero_count,
    ReqOrMom<MOM> req_count, uint32_t visits, uint32_t grp) {
    step_merged_body<INTEG, NL, 64, 1, false, false, MOM>(Pp, SO, OneGroup{{list, count, out, out_count, zero_count}, grp},
                                                          mom_of<MOM>(req_count), visits);
}

// The whole-wave phase in block-owned chunks (step_chunks.h; run_fused, api_render.cpp): at most
// 8 * kChunkClassBlocks blocks, the wave slots of the GPU at XRT_STEP_WAVES, each running `passes`
// passes of `visits` visits over the chunks it owns in the launch numbered rot, then adding the live
// slots it is left with to live_count for the host's poll.  A chunk is read and written by one block
// per launch, so the barrier between passes orders everything; launches are ordered by the stream.
template <int INTEG, int NL>
__global__ __launch_bounds__(kBlock, XRT_STEP_WAVES) void k_step_merged_chunks(
    const KParams* __restrict__ Pp, const StepObjs SO, const uint32_t* __restrict__ hdr, uint32_t* cnt, uint32_t* seg,
    uint32_t* live_count, uint32_t* zero_count, uint32_t visits, uint32_t passes, uint32_t rot) {
    step_merged_body<INTEG, NL, 64, 1, false, false, false>(Pp, SO, OwnedChunks{hdr, cnt, seg, live_count, zero_count, rot},
                                                            nullptr, visits | passes << 8);
}

// ---------------------------------------------------------------- launch dispatch ----
template <bool MOM, int INTEG, int SPW, int G, bool LANE, bool BVH = false, int WV = 0>
static void launch_merged_i(const KParams& P, const KParams* dP, const StepObjs& SO, const uint32_t* list,
                            const uint32_t* count, uint32_t* out, uint32_t* out_count, uint32_t* zero,
                            ReqOrMom<MOM> req_count, uint32_t visits, uint32_t part_live, size_t lds, uint32_t grp,
                            hipStream_t st) {
    // one block per per_block live entries of the fullest partition (part_iter strides over
    // any remainder, so an upper bound on the live count is all the grid needs), for each of
    // the partitions the launch's group holds
    const uint32_t per_block = (kBlock / 64) * SPW;
    const uint32_t blocks = (grp >> 8) * ((std::min(part_live, P.part_cap) + per_block - 1) / per_block);
    auto go = [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        // one of several groups (launch_step_merged has checked that the layout is the whole-wave one)
        if constexpr (SPW == 64 && G == 1 && !LANE && !BVH) {
            if (((grp >> 4) & 15u) > 1u) {
                hipLaunchKernelGGL((k_step_merged_group<INTEG, NL, MOM>), dim3(blocks), dim3(kBlock), lds, st, dP, SO, list, count,
                                   out, out_count, zero, req_count, visits, grp);
                return;
            }
        }
        hipLaunchKernelGGL((k_step_merged<INTEG, NL, SPW, G, LANE, BVH, WV, MOM>), dim3(blocks), dim3(kBlock), lds, st, dP, SO,
                           list, count, out, out_count, zero, req_count, visits);
    };
    if constexpr (BVH) with_const<1, 2>(P.n_lights, go);   // use_step_bvh: 1 or 2 lights
    else with_const<0, 1, 2, 3, 4>(P.n_lights, go);
}

// the moments builds leave out the XRT_LANE_TRACE experiment layout
template <bool MOM, int INTEG>
static void launch_merged_spw(const KParams& P, const KParams* dP, const StepObjs& SO, const uint32_t* list,
                              const uint32_t* count, uint32_t* out, uint32_t* out_count, uint32_t* zero,
                              ReqOrMom<MOM> req_count, uint32_t visits, uint64_t live, uint32_t part_live, size_t lds,
                              uint32_t grp, hipStream_t st) {
    const bool group = P.n_tris <= 64 && !(P.rflags & XRT_FLAG_NO_GROUP);   // group trace: 64-bit triangle masks
    const bool lane64 = group && exp_env("XRT_LANE_TRACE");   // experiment: per-lane traces, full waves
    (void)lane64;
    if (P.two_level) {   // use_step_bvh (never group traces: n_tris > 64)
#define XRT_BVH_CASE(SPWV) \
    launch_merged_i<MOM, INTEG, SPWV, 1, false, true>(P, dP, *P.sstep, list, count, out, out_count, zero, req_count, visits, \
                                                 part_live, lds, grp, st)
        switch (step_merged_spw(P, live)) {
            case 64: XRT_BVH_CASE(64); break;
            case 32: XRT_BVH_CASE(32); break;
            default:
                // below XRT_BVH_LOW_LIVE live slots (a frame's or a row shard's tail) the
                // XRT_BVH_LOW_WAVES build: more registers per wave, fewer spills
                if (live < XRT_BVH_LOW_LIVE)
                    launch_merged_i<MOM, INTEG, 16, 1, false, true, XRT_BVH_LOW_WAVES>(
                        P, dP, *P.sstep, list, count, out, out_count, zero, req_count, visits, part_live, lds, grp, st);
                else
                    XRT_BVH_CASE(16);
                break;
        }
#undef XRT_BVH_CASE
        return;
    }
#define XRT_MERGED_CASE(SPWV, GV, LV) \
    launch_merged_i<MOM, INTEG, SPWV, GV, LV>(P, dP, SO, list, count, out, out_count, zero, req_count, visits, part_live, lds, grp, st)
    switch (step_merged_spw(P, live)) {
        case 64:
            if constexpr (!MOM) {
                if (lane64) {
                    XRT_MERGED_CASE(64, 1, true);
                    break;
                }
            }
            XRT_MERGED_CASE(64, 1, false);
            break;
        case 32: if (group) XRT_MERGED_CASE(32, 2, true); else XRT_MERGED_CASE(32, 1, false); break;
        case 4: XRT_MERGED_CASE(4, 16, true); break;   // only with group traces (step_merged_spw)
        case 8: XRT_MERGED_CASE(8, 8, true); break;    // only with group traces (step_merged_spw)
        default: if (group) XRT_MERGED_CASE(16, 4, true); else XRT_MERGED_CASE(16, 1, false); break;
    }
#undef XRT_MERGED_CASE
}

// launch_step_merged's contract (launch.h); each unit instantiates its own MOM
template <bool MOM>
hipError_t launch_step_merged_as(const KParams& P, const KParams* dP, const StepObjs& SO, const uint32_t* list,
                                 const uint32_t* count, uint32_t* out, uint32_t* out_count, uint32_t* zero,
                                 ReqOrMom<MOM> req_count, uint32_t visits, uint64_t live, uint32_t live_part_max,
                                 uint32_t groups, uint32_t group, hipStream_t st) {
    if (group >= groups || !step_groups_eligible(P.n_part, groups)) return hipErrorInvalidValue;
    // groups exist for whole waves of one-level scenes traced by pair passes (k_step_merged_group)
    if (groups > 1 && (P.two_level || step_merged_spw(P, live) != 64 || exp_env("XRT_LANE_TRACE"))) return hipErrorInvalidValue;
    const uint32_t grp = step_group_arg(P.n_part, groups, group);
    const size_t lds = step_merged_lds_bytes(P);
    with_const<XRT_INTEGRATOR_DIRECT, XRT_INTEGRATOR_GI>(P.integrator, [&](auto integ) {   // use_step_merged / _bvh
        launch_merged_spw<MOM, decltype(integ)::value>(P, dP, SO, list, count, out, out_count, zero, req_count, visits, live,
                                                       live_part_max, lds, grp, st);
    });
    return hipGetLastError();
}
// the moments unit's instantiation (step_merged_mom.hip), which launch_step_merged forwards to
hipError_t launch_step_merged_mom(const KParams& P, const KParams* dP, const StepObjs& SO, const uint32_t* list,
                                  const uint32_t* count, uint32_t* out, uint32_t* out_count, uint32_t* zero,
                                  float2* mom, uint32_t visits, uint64_t live, uint32_t live_part_max,
                                  uint32_t groups, uint32_t group, hipStream_t st);

}  // namespace xrt
