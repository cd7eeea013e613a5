// step.hip — the fused schedule: trace and shading in one kernel, the scene in LDS
// (lscene.h), the path state in registers for `visits` segments per launch.
//   k_step     : one ray per lane; every scene kind and integrator, media included (medium.h)
//   k_step_tri : small triangle scenes (GI / Direct) with cooperative traces (coop_trace)
// The merged-trace triangle schedule (step_merged.h) and its speculative variant (spec.hip)
// take the scenes they are eligible for before these two.
#include <type_traits>

#include "launch.h"
#include "lscene.h"
#include "medium.h"
#include "path_common.h"

namespace xrt {

// WV: waves per SIMD the register budget is sized for (XRT_KSTEP_WAVES; the volumetric
// integrators also at 2, for launches with too few live slots to fill more: no spills)
// MOM (a variance render under XRT_FLAG_VAR_FUSED, xrt_render_var): an accepted sample also adds its
// luminance l and l * l to the slot's record {s1, s2}, which arrives in req_count's place (no step
// kernel reads req_count; k_shade<MOM>'s route, shade.hip) and was zeroed before seeding
// (render_impl).  Every sample ends in the `while (ended)` block: the one site.  The record is
// carried in registers for the launch, loaded and stored beside the pixel's sum (XRT_MOM_REGS,
// tuning.h; 0: a read-modify-write at the site, measured 2-5 % slower).
template <int SCN, int INTEG, int BS = kBlock, int WV = XRT_KSTEP_WAVES, bool MOM = false>
__global__ __launch_bounds__(BS, WV) void k_step(KParams P, const uint32_t* __restrict__ list,
                                                  const uint32_t* __restrict__ count, uint32_t* __restrict__ out,
                                                  uint32_t* out_count, uint32_t* zero_count,
                                                  std::conditional_t<MOM, float2*, uint32_t*> req_count, uint32_t visits) {
    extern __shared__ __attribute__((aligned(16))) f4 lds_step[];
    char* lb = reinterpret_cast<char*>(lds_step);
    const int tid = threadIdx.x;
    const LScene L = load_lscene(P, lb, tid, BS);
    __syncthreads();
    zero_parts(P, zero_count);
    const int lane = tid & 63;
    const PartIter it = part_iter(P, count, BS);
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const uint32_t i = base + tid;
        const uint32_t s = i < it.n ? list[it.p * P.part_cap + i] : 0;
        uint32_t st = i < it.n ? P.state[s] : ST_DONE;
        bool want_req = false;
        uint32_t g = 0;
        if (!(st & ST_DONE)) {
        // slot_load (path_common.h), open-coded: the call changes the volumetric kernels' instructions
        g = P.rng_g[s];
        Rng rng{P.ring + (size_t)s * kRing, P.rng_c[s]};
        uint32_t depth = P.depth[s];
        uint32_t k = P.sample_k[s];
        v3 thr = mk(1, 1, 1), rad = mk(0, 0, 0), o = mk(0, 0, 0), d = mk(0, 0, 0);
        if (!(st & ST_REGEN)) {
            thr = xyz(P.thr[s]), rad = xyz(P.rad[s]);
            o = xyz(P.ray_o[s]), d = xyz(P.ray_d[s]);
        }
        uint32_t nseg = 0, nsh = 0, nrej = 0, nstall = 0;
        const SlotPixel pix = slot_pixel_rowmajor(P, s);
        const uint32_t col = pix.col, row = pix.row;
        float* px = P.fb + 3 * ((size_t)col + (size_t)P.width * row);
        v3 acc = mk(px[0], px[1], px[2]);   // the pixel's running sum, in registers this launch
        float2 msum = make_float2(0.0f, 0.0f);   // MOM with XRT_MOM_REGS: the slot's record, carried like acc
        if constexpr (MOM && XRT_MOM_REGS) msum = req_count[s];
        rng.prefetch(g - rng.c);
        // VPT family: one event per iteration (kVptEvents) — a trace + surface interaction, or
        // ONE delta-tracking collision of a walk that continues across iterations in
        // registers — so lanes whose walks end early start their next segment (or sample)
        // while the others keep colliding, instead of idling until the wave's longest walk
        // ends.  Each lane's own sequence of operations and draws is unchanged.
        constexpr bool EV = vpt_family(INTEG) && kVptEvents;
        bool walking = false;
        float mt = 0.0f, mt1 = 0.0f;
        v3 tt = mk(1, 1, 1), sa = mk(0, 0, 0);
        for (uint32_t vis = 0; vis < visits; ++vis) {
            if ((st & ST_DONE) || (!walking && g - rng.c < kRngVisit)) break;
            bool ended = false, trace = true;
            if (EV && walking) {
                trace = false;
            } else if (st & ST_REGEN) {
                // next sample: sample_start (path_common.h), open-coded here and below: the call
                // changes the volumetric kernels' instructions
                st &= ~ST_REGEN;
                const float u = div_w(P, (float)(int)col + rng.next());
                const float v = div_h(P, (float)(int)row + rng.next());
                camera_ray(P, u, v, o, d);
                thr = mk(1, 1, 1), rad = mk(0, 0, 0);
                depth = 0;
                if (!one_hit(INTEG) && P.max_depth == 0) ended = true, trace = false;
            } else if (vpt_family(INTEG) && (st & ST_MEDIUM)) {
                trace = false;
            } else if (INTEG == XRT_INTEGRATOR_VPT_NEE && (st & ST_NEEWALK)) {
                // the previous launch suspended this path's NEE ratio tracking
                trace = false;
                if (nee_resume(P, s, thr, rad, rng, g) == 0) {
                    st &= ~ST_NEEWALK;
                    if (depth >= P.max_depth) ended = true;
                    else trace = true;
                }
            }
            bool walk = EV && walking;
            if (!walk) mt = 0.0f, mt1 = 0.0f, tt = mk(1, 1, 1), sa = mk(0, 0, 0);
            if (vpt_family(INTEG) && (st & ST_MEDIUM)) {
                st &= ~ST_MEDIUM;
                const f4 m1 = P.med[s], m2 = P.med2[s];
                mt = m1.x, mt1 = m1.y, sa = mk(m1.z, m1.w, m2.w), tt = xyz(m2);
                walk = true;
            }
            if (trace) {
                ++nseg;
                HitRec h;
                closest_l<SCN>(P, L, o, d, h);
                Surf S;
                const int obj = surface_l<SCN>(L, o, d, h, S);
                if (INTEG == XRT_INTEGRATOR_DIRECT) {
                    // DirectIntegrator::integrate (Src/integrator.h:82-119)
                    if (obj < 0) {
                        rad = mk((float)0.18, (float)0.18, (float)0.18);
                    } else if (L.obj[obj].light >= 0) {
                        rad = light_Le(L.light[L.obj[obj].light], S.ns, d);
                    } else {
                        const DObj& ob = L.obj[obj];
                        for (int l = 0; l < P.n_lights; ++l) {
                            v3 wi = mk(0, 0, 0);
                            float tmax = 0.0f, pdf = 0.0f;
                            const v3 Lv = light_sample(L.light[l], S.pos, wi, pdf, tmax, rng);
                            if (pdf == 0.0f) continue;
                            const float bias = 0.01f;
                            ++nsh;
                            const bool vis = !occluded_l<SCN>(P, L, S.pos + S.ng * bias, wi, tmax - bias);
                            const float cosv = smax(0.0f, dot(S.ng, wi));
                            const v3 fr = eval_bxdf(ob);
                            rad = rad + div3s(((fr * (float)vis) * Lv) * cosv, pdf);
                        }
                    }
                    ended = true;
                } else if (vpt_family(INTEG)) {
                    // VolumePathTracing::integrate loop body (Src/integrator.h:418-469);
                    // VolumePathTracingNEE (:497-581): Le only at depth 0
                    if (obj < 0) {
                        rad = rad + (thr * mk(0.0f, 0.0f, 0.0f)) * (float)(depth != 0);
                        ended = true;
                    } else {
                        bool alive = true;
                        if (depth > 0) {   // russian_roulette (path_common.h) with the quotient through div3s
                            const float pr = smin((thr.x + thr.y + thr.z) / 3.0f, 1.0f);
                            if (rng.next() >= pr) alive = false, ended = true;
                            else thr = div3s(thr, pr);   // thr / Vec3f(pr): one division when achromatic
                        }
                        const DObj& ob = L.obj[obj];
                        if (alive && ob.light >= 0) {
                            if (INTEG == XRT_INTEGRATOR_VPT || depth == 0)
                                rad = rad + thr * light_Le(L.light[ob.light], S.ns, d);
                            alive = false, ended = true;
                        }
                        if (alive) {
                            if (ob.medium >= 0) {
                                mt = h.t, mt1 = h.t1;
                                if (P.medium.kind == XRT_MEDIUM_HETEROGENEOUS)
                                    sa = ld3(P.medium.absorption) * medium_density(P.medium, ray_at(o, d, mt));
                                walk = true;
                            } else {
                                ++nstall;   // see k_shade: the reference never advances this ray
                                ended = true;
                            }
                        }
                    }
                } else if (INTEG == XRT_INTEGRATOR_NORMAL) {
                    // NormalIntegrator::integrate (Src/integrator.h:28-37): 0.5 * (ns + 1)
                    if (obj >= 0) rad = normal_color(S.ns);
                    ended = true;
                } else {
                    // GIIntegrator::integrate loop body (Src/integrator.h:214-284);
                    // IndirectIntegrator (Src/integrator.h:138-185): no light sampling, Le at
                    // every depth
                    if (obj < 0) {
                        rad = rad + thr * mk(0.0f, 0.0f, 0.0f);
                        ended = true;
                    } else {
                        bool alive = true;
                        if (depth > 0) {   // russian_roulette (path_common.h), open-coded: the call adds SGPR spills
                            const float pr = smin((thr.x + thr.y + thr.z) / 3.0f, 1.0f);
                            if (rng.next() >= pr) alive = false, ended = true;
                            else thr = thr / mk(pr, pr, pr);
                        }
                        const DObj& ob = L.obj[obj];
                        if (alive && ob.light >= 0) {
                            if (depth == 0 || INTEG == XRT_INTEGRATOR_INDIRECT)
                                rad = rad + thr * light_Le(L.light[ob.light], S.ns, d);
                            alive = false, ended = true;
                        }
                        if (alive) {
                            v3 directL = mk(0, 0, 0);
                            for (int l = 0; l < (INTEG == XRT_INTEGRATOR_GI ? P.n_lights : 0); ++l) {
                                v3 L_light = mk(0, 0, 0);
                                v3 wi = mk(0, 0, 0);
                                float tmax = 0.0f, pdf = 0.0f;
                                const v3 Lv = light_sample(L.light[l], S.pos, wi, pdf, tmax, rng);
                                if (pdf == 0.0f) continue;
                                const float bias = 0.01f;
                                ++nsh;
                                const bool vis = !occluded_l<SCN>(P, L, S.pos + S.ng * bias, wi, tmax - bias);
                                const float cosv = smax(0.0f, dot(S.ng, wi));
                                const v3 fr = eval_bxdf(ob);
                                L_light = L_light + (((fr * (float)vis) * Lv) * cosv) / pdf;
                                directL = directL + L_light;
                            }
                            if (INTEG == XRT_INTEGRATOR_GI) rad = rad + thr * directL;
                            // lambert_bounce (path_common.h), open-coded: with the call k_step<SCN_SPHERE, GI>
                            // measured slower than the parent's own spread in both repetitions
                            float pdf = 1.0f;
                            v3 nd = mk(0, 0, 0), fr = mk(0, 0, 0);
                            if (ob.material == 1) {
                                nd = lambert_sample(S, rng);
                                pdf = 1.0f / (2.0f * kPI);
                                fr = eval_bxdf(ob);
                            }
                            const float cosv = smax(0.0f, dot(nd, S.ng));
                            thr = thr * ((fr * cosv) / pdf);
                            o = S.pos + S.ng * 0.01f;
                            d = nd;
                            ++depth;
                            if (depth >= P.max_depth) ended = true;
                        }
                    }
                }
            }
            if (vpt_family(INTEG) && walk) {
                v3 pos, dir, tm;
                const int r = P.medium.kind != XRT_MEDIUM_HETEROGENEOUS
                                  ? homog_track(P, o, d, thr, mt, mt1, rng, pos, dir, tm)
                              : EV ? delta_step(P, o, d, thr, mt, mt1, tt, sa, rng, g, pos, dir, tm)
                                   : delta_track(P, o, d, thr, mt, mt1, tt, sa, rng, g, pos, dir, tm);
                walking = EV && r == 3;   // null collision: the walk goes on next iteration
                if (r == 3) {
                } else if (r == 2) {
                    st |= ST_MEDIUM;
                    P.med[s] = make_float4(mt, mt1, sa.x, sa.y);
                    P.med2[s] = make_float4(tt.x, tt.y, tt.z, sa.z);
                } else {
                    // VolumePathTracingNEE: light sample at a scattering event, before the
                    // ray advances (Src/integrator.h:537-572)
                    const int nr = (INTEG == XRT_INTEGRATOR_VPT_NEE && r == 1)
                                       ? nee_medium<SCN>(P, L, s, pos, d, thr * tm, rad, rng, g, nsh)
                                       : 0;
                    o = pos, d = dir;
                    thr = thr * tm;
                    if (r == 1) ++depth;
                    if (nr == 2) st |= ST_NEEWALK;   // resumes at the next launch (RNG words ran out)
                    else if (depth >= P.max_depth) ended = true;
                }
            }
            // finish the sample (Src/renderer.cpp:55-75) and start the next one right away:
            // its jitter draws are still in the prefetch buffer (a segment draws <= 13 of the
            // >= 16 words it starts with), so the next segment opens with the trace while
            // the words it needs next are loading.
            while (ended) {
                ended = false;
                const v3 r = rad / 1.0f;
                // radiance_invalid (path_common.h), open-coded: the call changes the volumetric kernels
                if (__builtin_isnan(r.x) || __builtin_isnan(r.y) || __builtin_isnan(r.z) || __builtin_isinf(r.x) ||
                    __builtin_isinf(r.y) || __builtin_isinf(r.z) || r.x < 0.0f || r.y < 0.0f || r.z < 0.0f) {
                    ++nrej;
                } else {
                    acc = acc + r;
                    if constexpr (MOM) {   // s1 = s1 + l, s2 = s2 + l * l (include/xrt.h, xrt_render_var)
                        const float l = luminance(r);
                        if constexpr (XRT_MOM_REGS) {
                            msum.x = msum.x + l, msum.y = msum.y + l * l;
                        } else {
                            float2 m = req_count[s];
                            m.x = m.x + l, m.y = m.y + l * l;
                            req_count[s] = m;
                        }
                    }
                }
                ++k;
                if (k >= P.spp) {
                    st = ST_DONE;
                } else if (!one_hit(INTEG) && P.max_depth == 0) {
                    (void)rng.next(), (void)rng.next();   // the next sample's jitter; radiance 0
                    rad = mk(0, 0, 0);
                    ended = true;
                } else {
                    const float u = div_w(P, (float)(int)col + rng.next());
                    const float v = div_h(P, (float)(int)row + rng.next());
                    camera_ray(P, u, v, o, d);
                    thr = mk(1, 1, 1), rad = mk(0, 0, 0);
                    depth = 0;
                }
            }
            if (!EV || rng.nb < kVptEventPrefetch) rng.prefetch(g - rng.c);
        }
        if (EV && walking) {   // the launch ended mid-walk: resume it like a suspended one
            st |= ST_MEDIUM;
            P.med[s] = make_float4(mt, mt1, sa.x, sa.y);
            P.med2[s] = make_float4(tt.x, tt.y, tt.z, sa.z);
        }
        // slot_store (path_common.h), open-coded as slot_load above
        px[0] = acc.x, px[1] = acc.y, px[2] = acc.z;
        if constexpr (MOM && XRT_MOM_REGS) req_count[s] = msum;
        // RNG refill (words ahead < rng_keep <= 624): twisted by this wave below
        want_req = !(st & (ST_DONE | ST_RNGREQ)) && g - rng.c < P.rng_keep;
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
        if (nstall) P.c_stall[s] += nstall;
        }
        // live list of the next round (partitioned, one atomic per wave), then the wave's
        // refills in-line (as k_step_merged: no k_refill launch between step launches)
        wave_append(!(st & ST_DONE), s, out + it.p * P.part_cap, out_count + it.p, lane);
        if (kstep_refill_off(P, BS)) {   // wave_refill staging: the wave's kMT words after the scene
            uint32_t* rbuf = reinterpret_cast<uint32_t*>(lb + kstep_refill_off(P, BS)) + (tid >> 6) * kMT;
            wave_refill(P, want_req, s, g, lane, rbuf);
        } else {
            // sphere-BVH scenes: twisted from global memory (L2), no LDS buffer beside the
            // scene's ~45 KB (3 blocks per CU instead of 2)
            uint32_t gn = g;
            wave_refill(want_req, s, gn, P.ring, lane);
            if (want_req) P.rng_g[s] = gn;
        }
    }
    (void)req_count;
}

// ======================================================= cooperative triangle trace ====
// For triangle scenes the rays of a wave are incoherent after the first bounce: tracing one
// ray per lane, a wave pays for every object any of its 64 rays needs (measured on C2:
// ~29 triangle tests per wave per trace while a ray needs ~5).  The cooperative trace
// instead culls each ray against the object boxes, lays the (ray, triangle) pairs that
// survive out in one flat index space (exclusive scan over the lanes; each lane writes its
// pairs into an LDS list, 512 per chunk) and tests 64 pairs per pass — every lane busy.  Results are merged per ray in LDS: closest hit = atomicMin
// of (t bits << 32 | triangle index), i.e. smallest t and, on a tie, the triangle the
// reference's in-order `t < best` loop keeps (triangles are packed in Scene iteration
// order); then the owner lane recomputes u, v of its winner with the same Moller-Trumbore
// ops.  Shadow rays set an occlusion flag.  Requires n_objs <= 32 (object masks).
struct CoopWave {
    f4 ro[64];                     // ray origin, w = tmax (shadow rays)
    f4 rd[64];
    unsigned long long best[64];   // closest: packed (t, tri); shadow: != 0 occluded
    uint32_t pair[512];            // expanded pairs of the current chunk: owner << 24 | tri
};
constexpr int kCoopMaxObjs = 32;
constexpr uint32_t kCoopCap = 512;

template <bool SHADOW>
__device__ __forceinline__ unsigned long long coop_trace(const KParams& P, const LScene& L, CoopWave& W, int lane,
                                                         bool want, v3 o, v3 d, float tmax) {
    uint32_t m = 0, n = 0;
    if (want) {
        const v3 inv = rcp3(d);
        for (int ob = 0; ob < P.n_objs; ++ob) {
            const DObjBox B = L.box[ob];
            if (SHADOW && B.count_occ >= 0) continue;   // area-light objects never occlude
            if (box_overlap(o, inv, B, SHADOW ? tmax : kINF)) m |= 1u << ob, n += B.count_occ & 0x7fffffff;
        }
    }
    uint32_t incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const uint32_t total = __shfl(incl, 63);
    const uint32_t pre = incl - n;
    W.ro[lane] = make_float4(o.x, o.y, o.z, tmax);
    W.rd[lane] = make_float4(d.x, d.y, d.z, 0.0f);
    W.best[lane] = SHADOW ? 0ull : ~0ull;
    for (uint32_t c0 = 0; c0 < total; c0 += kCoopCap) {
        // expand this lane's pairs that fall into the chunk [c0, c0 + kCoopCap)
        if (n && pre < c0 + kCoopCap && pre + n > c0) {
            uint32_t pos = pre, mm = m;
            while (mm) {
                const int ob = __builtin_ctz(mm);
                mm &= mm - 1;
                const DObjBox B = L.box[ob];
                const uint32_t c = B.count_occ & 0x7fffffff;
                const uint32_t lo = max(pos, c0), hi = min(pos + c, c0 + kCoopCap);
                for (uint32_t q = lo; q < hi; ++q) W.pair[q - c0] = ((uint32_t)lane << 24) | (B.first + (q - pos));
                pos += c;
            }
        }
        wave_sync();
        const uint32_t cnt = min(kCoopCap, total - c0);
        for (uint32_t j = lane; j < cnt; j += 64) {
            const uint32_t e = W.pair[j];
            const int r = (int)(e >> 24), k = (int)(e & 0xffffffu);
            const f4 A = W.ro[r];
            float t, u, v;
            if (ray_tri(xyz(A), xyz(W.rd[r]), xyz(L.tri[3 * k]), xyz(L.tri[3 * k + 1]), xyz(L.tri[3 * k + 2]), t, u,
                        v)) {
                if (SHADOW) {
                    if (t < A.w) W.best[r] = 1ull;
                } else {
                    atomicMin(&W.best[r], ((unsigned long long)__float_as_uint(t) << 32) | (uint32_t)k);
                }
            }
        }
        wave_sync();
    }
    return W.best[lane];
}

__device__ __forceinline__ void coop_closest(const KParams& P, const LScene& L, CoopWave& W, int lane, bool want, v3 o,
                                             v3 d, HitRec& h) {
    const unsigned long long b = coop_trace<false>(P, L, W, lane, want, o, d, kINF);
    h.t = kINF, h.u = h.v = 0.0f, h.code = -1, h.surf = -1, h.dp = -1, h.t1 = kINF;
    h.st = h.su = h.sv = h.du = h.dv = 0.0f;
    if (want && b != ~0ull) {
        const int k = (int)(uint32_t)b;
        float t, u, v;
        (void)ray_tri(o, d, xyz(L.tri[3 * k]), xyz(L.tri[3 * k + 1]), xyz(L.tri[3 * k + 2]), t, u, v);
        h.t = t, h.u = u, h.v = v, h.code = k;
    }
}

// k_step for triangle scenes (GI / Direct) with cooperative traces: the same per-slot
// sequence as k_step, arranged so every trace is reached by the whole wave (per-lane
// activity flags instead of divergent control flow around the traces).
// MOM: as k_step's.
template <int INTEG, bool MOM = false>
__global__ __launch_bounds__(kBlock, XRT_STEP_WAVES) void k_step_tri(const KParams* __restrict__ Pp,
                                                                      const uint32_t* __restrict__ list,
                                                                      const uint32_t* __restrict__ count,
                                                                      uint32_t* __restrict__ out, uint32_t* out_count,
                                                                      uint32_t* zero_count,
                                                                      std::conditional_t<MOM, float2*, uint32_t*> req_count,
                                                                      uint32_t visits) {
    // KParams lives in device memory here (one copy per render): fields are fetched with
    // scalar loads when needed instead of pinning ~150 SGPRs of kernel arguments
    const KParams& P = *Pp;
    extern __shared__ __attribute__((aligned(16))) f4 lds_step[];
    char* lb = reinterpret_cast<char*>(lds_step);
    // load_lscene (lscene.h) for a triangle scene, open-coded: the call adds spills and scratch here
    const StepLayout Lo = step_layout(P);
    LScene L;
    L.tri = reinterpret_cast<const f4*>(lb + Lo.tri);
    L.tng = reinterpret_cast<const f4*>(lb + Lo.tng);
    L.nrm = reinterpret_cast<const f4*>(lb + Lo.nrm);
    L.box = reinterpret_cast<const DObjBox*>(lb + Lo.box);
    L.sph = reinterpret_cast<const f4*>(lb + Lo.sph);
    L.bx = reinterpret_cast<const f4*>(lb + Lo.bx);
    L.obj = reinterpret_cast<const DObj*>(lb + Lo.obj);
    L.light = reinterpret_cast<const DLight*>(lb + Lo.light);
    L.sobj = reinterpret_cast<const int*>(lb + Lo.sobj);
    const int tid = threadIdx.x, lane = tid & 63;
    CoopWave& W = reinterpret_cast<CoopWave*>(lb + ((Lo.total + 15u) & ~15u))[tid >> 6];
    lds_copy(const_cast<f4*>(L.tri), P.tri, 3 * P.n_tris, tid);
    lds_copy(const_cast<f4*>(L.tng), P.tri_ng, P.n_tris, tid);
    lds_copy(const_cast<f4*>(L.nrm), P.tri_nrm, 3 * P.n_tris, tid);
    lds_copy(const_cast<DObjBox*>(L.box), P.obj_box, P.n_objs, tid);
    lds_copy(const_cast<DObj*>(L.obj), P.objs, P.n_objs, tid);
    lds_copy(const_cast<DLight*>(L.light), P.lights, P.n_lights, tid);
    __syncthreads();
    zero_parts(P, zero_count);
    const PartIter it = part_iter(P, count, kBlock);
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const uint32_t i = base + tid;
        const uint32_t s = i < it.n ? list[it.p * P.part_cap + i] : 0;
        uint32_t st = i < it.n ? P.state[s] : ST_DONE;
        const bool live = !(st & ST_DONE);
        uint32_t g = 0, depth = 0, k = 0;
        Rng rng{P.ring + (size_t)s * kRing, 0};
        v3 thr = mk(1, 1, 1), rad = mk(0, 0, 0), o = mk(0, 0, 0), d = mk(0, 0, 0), acc = mk(0, 0, 0);
        const SlotPixel pix = slot_pixel_rowmajor(P, s);
        const uint32_t col = pix.col, row = pix.row;
        float* px = P.fb + 3 * ((size_t)col + (size_t)P.width * row);
        if (live) slot_load(P, s, st, px, g, rng, depth, k, thr, rad, o, d, acc);
        float2 msum = make_float2(0.0f, 0.0f);   // MOM with XRT_MOM_REGS: the slot's record, carried like acc
        if constexpr (MOM && XRT_MOM_REGS) {
            if (live) msum = req_count[s];
        }
        uint32_t nseg = 0, nsh = 0, nrej = 0;
        for (uint32_t vis = 0; vis < visits; ++vis) {
            const bool act = live && !(st & ST_DONE) && g - rng.c >= kRngVisit;
            if (!__ballot(act)) break;
            if (act && (st & ST_REGEN)) {
                // first sample of the slot: jitter draws + camera ray (Src/renderer.cpp:44-50)
                st &= ~ST_REGEN;
                const float jx = rng.next();
                const float jy = rng.next();
                sample_start(P, col, row, jx, jy, o, d, thr, rad, depth);
            }
            bool ended = false, alive = false;
            if (!one_hit(INTEG) && P.max_depth == 0) ended = act;   // bounce loop never runs
            const bool ext = act && !ended;
            HitRec h;
            coop_closest(P, L, W, lane, ext, o, d, h);
            // SurfaceInfo of a triangle hit: position, face normal; the shading normal (for
            // Le) and the dpdu/dpdv frame (for the BSDF) are rebuilt from (tri, u, v) where used
            Surf S;
            S.pos = S.ng = S.ns = S.dpdu = S.dpdv = mk(0, 0, 0);
            int obj = -1;
            const int hk = h.code;
            const float hu = h.u, hv = h.v;
            if (ext) {
                ++nseg;
                if (hk >= 0) {
                    S.pos = ray_at(o, d, h.t);
                    S.ng = xyz(L.tng[hk]);
                    obj = __float_as_int(L.tri[3 * hk].w);
                }
                if (INTEG == XRT_INTEGRATOR_DIRECT) {
                    // DirectIntegrator::integrate (Src/integrator.h:82-119)
                    if (obj < 0) {
                        rad = mk((float)0.18, (float)0.18, (float)0.18);
                        ended = true;
                    } else if (L.obj[obj].light >= 0) {
                        rad = light_Le(L.light[L.obj[obj].light], tri_ns_l(L, hk, hu, hv), d);
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
                        if (depth > 0 && !russian_roulette(thr, rng)) alive = false, ended = true;
                        if (alive && L.obj[obj].light >= 0) {
                            if (depth == 0)
                                rad = rad + thr * light_Le(L.light[L.obj[obj].light], tri_ns_l(L, hk, hu, hv), d);
                            alive = false, ended = true;
                        }
                    }
                }
            }
            // next-event estimation: one cooperative shadow trace per light, in light order
            v3 directL = mk(0, 0, 0);
            for (int l = 0; l < P.n_lights; ++l) {
                v3 wi = mk(0, 0, 0), Lv = mk(0, 0, 0);
                float tmax = 0.0f, pdf = 0.0f;
                if (alive) Lv = light_sample(L.light[l], S.pos, wi, pdf, tmax, rng);
                const bool sh = alive && pdf != 0.0f;
                const float bias = 0.01f;
                const bool occ = coop_trace<true>(P, L, W, lane, sh, S.pos + S.ng * bias, wi, tmax - bias) != 0;
                if (sh) {
                    ++nsh;
                    const float cosv = smax(0.0f, dot(S.ng, wi));
                    const v3 fr = eval_bxdf(L.obj[obj]);
                    const v3 c = (((fr * (float)!occ) * Lv) * cosv) / pdf;
                    if (INTEG == XRT_INTEGRATOR_DIRECT) {
                        rad = rad + c;
                    } else {
                        const v3 L_light = mk(0, 0, 0) + c;
                        directL = directL + L_light;
                    }
                }
            }
            if (alive) {
                if (INTEG == XRT_INTEGRATOR_DIRECT) {
                    ended = true;
                } else {
                    rad = rad + thr * directL;
                    const DObj& ob = L.obj[obj];
                    if (ob.material == 1) onb(tri_ns_l(L, hk, hu, hv), S.dpdu, S.dpdv);   // the BSDF's frame
                    lambert_bounce(ob, S, rng, thr, o, d);
                    ++depth;
                    if (depth >= P.max_depth) ended = true;
                }
            }
            // finish the sample and start the next one (see k_step)
            while (ended) {
                ended = false;
                const v3 r = rad / 1.0f;
                if (radiance_invalid(r)) {
                    ++nrej;
                } else {
                    acc = acc + r;
                    if constexpr (MOM) {
                        const float l = luminance(r);
                        if constexpr (XRT_MOM_REGS) {
                            msum.x = msum.x + l, msum.y = msum.y + l * l;
                        } else {
                            float2 m = req_count[s];
                            m.x = m.x + l, m.y = m.y + l * l;
                            req_count[s] = m;
                        }
                    }
                }
                ++k;
                if (k >= P.spp) {
                    st = ST_DONE;
                } else if (!one_hit(INTEG) && P.max_depth == 0) {
                    (void)rng.next(), (void)rng.next();
                    rad = mk(0, 0, 0);
                    ended = true;
                } else {
                    const float jx = rng.next();
                    const float jy = rng.next();
                    sample_start(P, col, row, jx, jy, o, d, thr, rad, depth);
                }
            }
            if (act) rng.prefetch(g - rng.c);
        }
        bool want_req = false;   // the slot's ring runs low: twisted below
        if (live) want_req = slot_store(P, s, st, px, g, rng, depth, k, thr, rad, o, d, acc, nseg, nsh, nrej, 0u);
        if constexpr (MOM && XRT_MOM_REGS) {
            if (live) req_count[s] = msum;
        }
        wave_append(live && !(st & ST_DONE), s, out + it.p * P.part_cap, out_count + it.p, lane);
        // the wave's refills in-line through its trace scratch (idle now)
        static_assert(sizeof(CoopWave) >= kMT * sizeof(uint32_t), "refill staging");
        wave_refill(P, want_req, s, g, lane, reinterpret_cast<uint32_t*>(&W));
    }
    (void)req_count;
}

size_t step_lds_bytes(const KParams& P) {
    if (P.scene_kind == SCN_TRI && !P.small_tri) return 0;   // needs the per-object boxes
    if (P.n_tris > 65536 || P.n_sph > 65536 || P.n_box > 65536 || P.n_objs > 65536) return 0;
    const size_t total = step_layout(P).total;
    return total <= kStepLds ? (total + 15) / 16 * 16 : 0;
}

// k_step's dynamic LDS: the scene carve, plus each wave's refill staging buffer where the
// in-line refill is staged through LDS (kstep_refill_off).  The staging sits outside the
// kStepLds scene budget (at most 64 KiB + 10 KiB per 256-thread block, within gfx950's
// 160 KiB per workgroup).
static size_t kstep_lds_bytes(const KParams& P, int bs) {
    const size_t off = kstep_refill_off(P, bs);
    return off ? off + (size_t)(bs / 64) * kMT * 4 : step_lds_bytes(P);
}

bool use_step_tri(const KParams& P) {
    return P.scene_kind == SCN_TRI && P.small_tri && P.n_objs <= kCoopMaxObjs &&
           (P.integrator == XRT_INTEGRATOR_GI || P.integrator == XRT_INTEGRATOR_DIRECT) && !exp_env("XRT_NO_COOP") &&
           ((step_layout(P).total + 15u) & ~15u) + (kBlock / 64) * sizeof(CoopWave) <= kStepLds;
}

// MOM: the moments builds, the slots' records in req_count's place
template <bool MOM>
static hipError_t launch_step_t(const KParams& P, const KParams* dP, const uint32_t* list, const uint32_t* count,
                                uint32_t* out, uint32_t* out_count, uint32_t* zero,
                                std::conditional_t<MOM, float2*, uint32_t*> req_count, uint32_t visits, uint32_t blocks,
                                uint64_t live, bool tri, hipStream_t st) {
    if (!step_lds_bytes(P)) return hipErrorInvalidValue;
    if (P.n_part == 0 || blocks % P.n_part != 0) return hipErrorInvalidValue;   // part_iter's grid contract
    if (tri) {   // use_step_tri: GI or Direct
        const size_t lds = ((step_layout(P).total + 15u) & ~15u) + (kBlock / 64) * sizeof(CoopWave);
        return with_const<XRT_INTEGRATOR_DIRECT, XRT_INTEGRATOR_GI>(P.integrator, [&](auto integ) {
            hipLaunchKernelGGL((k_step_tri<decltype(integ)::value, MOM>), dim3(blocks), dim3(kBlock), lds, st, dP, list, count,
                               out, out_count, zero, req_count, visits);
            return hipGetLastError();
        });
    }
    return with_scene_kind(P.scene_kind, [&](auto scn) {
        return with_integrator(P.integrator, [&](auto integ) {
            constexpr int SCN = decltype(scn)::value, I = decltype(integ)::value;
            // Sphere-BVH scenes (C3) keep ~45 KB of BVH and spheres in LDS, so 256-thread blocks stop
            // at 3 per CU (3 waves per SIMD); 512-thread blocks share one copy between 8 waves
            // (4 waves per SIMD, the VGPR limit).  Same partitions, same results.
            if constexpr (I == XRT_INTEGRATOR_DIRECT)
                if (SCN == SCN_SPHERE && P.n_snode > 0 && kStepBlock512) {
                    // the grid must stay a multiple of n_part (part_iter: block b serves partition b % n_part
                    // and chunk b / n_part of gridDim / n_part chunks)
                    const uint32_t chunks = std::max(1u, blocks / P.n_part);
                    hipLaunchKernelGGL((k_step<SCN, I, 512, XRT_KSTEP_WAVES, MOM>), dim3(P.n_part * ((chunks + 1) / 2)), dim3(512),
                                       kstep_lds_bytes(P, 512), st, P, list, count, out, out_count, zero, req_count, visits);
                    return hipGetLastError();
                }
            const size_t lds = kstep_lds_bytes(P, kBlock);
            // volumetric walks with fewer live slots than 2 waves per SIMD hold (a row shard of a
            // multi-GPU frame, a frame's tail): the 2-wave build, whose registers hold the walk without
            // spilling (C5 shard 0 of 8: 43.9 -> 41.9 ms; a full frame stays at 4 waves per SIMD)
            if constexpr (I == XRT_INTEGRATOR_VPT || I == XRT_INTEGRATOR_VPT_NEE)
                if (live < kVptLowLive) {
                    hipLaunchKernelGGL((k_step<SCN, I, kBlock, 2, MOM>), dim3(blocks), dim3(kBlock), lds, st, P, list, count, out,
                                       out_count, zero, req_count, visits);
                    return hipGetLastError();
                }
            hipLaunchKernelGGL((k_step<SCN, I, kBlock, XRT_KSTEP_WAVES, MOM>), dim3(blocks), dim3(kBlock), lds, st, P, list, count, out, out_count, zero,
                               req_count, visits);
            return hipGetLastError();
        });
    });
}

hipError_t launch_step(const KParams& P, const KParams* dP, const uint32_t* list, const uint32_t* count, uint32_t* out,
                       uint32_t* out_count, uint32_t* zero, uint32_t* req_count, uint32_t visits, uint32_t blocks,
                       uint64_t live, bool tri, hipStream_t st, float2* mom) {
    if (mom) return launch_step_t<true>(P, dP, list, count, out, out_count, zero, mom, visits, blocks, live, tri, st);
    return launch_step_t<false>(P, dP, list, count, out, out_count, zero, req_count, visits, blocks, live, tri, st);
}

}  // namespace xrt
