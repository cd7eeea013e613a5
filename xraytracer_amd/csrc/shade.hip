// shade.hip — the shade pass of the wavefront schedule.
//
// One path slot per pixel of the shard.  Each iteration runs two passes over a compacted
// slot list:
//   k_shade : per slot — resolve last bounce's NEE (shadow results), shade the hit record
//             (RR, emitter, NEE light samples -> shadow rays, Lambert BSDF sample ->
//             extension ray), finalize a finished sample into the framebuffer and
//             regenerate the pixel's next camera ray; ballot/prefix-sum compaction of the
//             slots that still have rays to trace.
//   k_trace : (trace.hip) closest-hit for extension rays and any-hit for shadow rays.
// Per-pixel RNG is an exact restatement of the reference's std::mt19937 stream; a pixel's
// samples run in order (sample k+1 starts in the same k_shade call that finalises k), so
// every pixel consumes its stream exactly as NormalRenderer::doRender does
// (Src/renderer.cpp:29-81).
#include "launch.h"
#include "lscene.h"
#include "medium.h"
#include "path_common.h"

namespace xrt {

// =================================================================== k_shade ====
// MOM (a variance render, xrt_render_var): the sample a slot finishes also adds its luminance l and
// l * l to the slot's record mom[s] = {s1, s2}, which the slot's very first visit zeroes (k_finish_var,
// frame.hip, turns the records into the variance plane).  The records take the place of req_count,
// which k_shade does not read: a member more in KParams or an argument more would move the
// arguments behind it, the hidden ones included, and with them instructions of every build.
template <int SCN, int INTEG, bool MOM = false>
__global__ __launch_bounds__(kBlock, XRT_SHADE_WAVES) void k_shade(KParams P, const uint32_t* __restrict__ list,
                                                   const uint32_t* __restrict__ count, uint32_t* __restrict__ out,
                                                   uint32_t* out_count,
                                                   std::conditional_t<MOM, float2*, uint32_t*> req_count_or_mom) {
    float2* mom = nullptr;
    if constexpr (MOM) mom = req_count_or_mom;
    __shared__ __attribute__((aligned(16))) uint32_t rbuf[kBlock / 64][kMT];   // wave_refill staging
    const PartIter it = part_iter(P, count, kBlock);
    const int tid = threadIdx.x, lane = tid & 63;
    // the two-level trace that follows appends to zeroed deep-queue counters (instead of a
    // memset launch per iteration); the previous iteration's deep walk is done by now
    if (P.two_level && P.deep_count && blockIdx.x == 0)
        for (uint32_t q = tid; q < 3 * kMaxParts; q += kBlock) P.deep_count[q] = 0;
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const uint32_t i = base + tid;
        const bool valid = i < it.n;
        const uint32_t s = valid ? list[it.p * P.part_cap + i] : 0;
        const uint32_t g = valid ? P.rng_g[s] : 0;
        Rng rng{P.ring + (size_t)s * kRing, valid ? P.rng_c[s] : 0};
        uint32_t st = valid ? P.state[s] : ST_DONE;
        // RNG words: below kRngMin the wave twists the slot's next block at the end of this
        // launch (wave_refill below; the block overwrites ring words < g - 624 <= c, all
        // drawn); below kRngVisit the slot sits this launch out
        const uint32_t avail = g - rng.c;
        const bool want_req = valid && avail < kRngMin;
        const bool go = valid && avail >= kRngVisit;
        if (go) {
            rng.prefetch(avail);
            uint32_t depth = P.depth[s];
            uint32_t k = P.sample_k[s];
            v3 thr = xyz(P.thr[s]), rad = xyz(P.rad[s]);
            v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
            uint32_t nseg = 0, nsh = 0, nrej = 0, nstall = 0;
            bool finalize = false;

            // ---- 1. resolve the previous bounce's NEE with the shadow-ray results
            if (st & ST_NEE) {
                const uint32_t smask = (st >> ST_SHADOW_SHIFT) & 0xffu;
                const uint32_t occ = smask ? P.occ[s] : 0u;
                if (INTEG == XRT_INTEGRATOR_DIRECT) {
                    // radiance += vis * fr * L * cos / pdf per light (Src/integrator.h:95-109)
                    for (int l = 0; l < P.n_lights; ++l) {
                        if (!(smask & (1u << l))) continue;
                        const v3 c = (occ & (1u << l)) ? mk(0, 0, 0) : xyz(P.sh_c[(size_t)l * P.n_slots + s]);
                        rad = rad + c;
                    }
                } else {
                    // L_light = 0 + vis*fr*L*cos/pdf; directL += L_light; radiance += thr*directL
                    // (Src/integrator.h:249-269)
                    v3 directL = mk(0, 0, 0);
                    for (int l = 0; l < P.n_lights; ++l) {
                        if (!(smask & (1u << l))) continue;
                        const v3 c = (occ & (1u << l)) ? mk(0, 0, 0) : xyz(P.sh_c[(size_t)l * P.n_slots + s]);
                        directL = directL + (mk(0, 0, 0) + c);
                    }
                    rad = rad + xyz(P.thr_prev[s]) * directL;
                }
                st &= ~(ST_NEE | (0xffu << ST_SHADOW_SHIFT));
                if (st & ST_END) finalize = true;
            }

            // ---- 2. shade the traced extension ray (or resume a suspended medium walk)
            if (vpt_family(INTEG) && (st & (ST_RAY | ST_MEDIUM | ST_NEEWALK))) {
                // VolumePathTracing::integrate loop body (Src/integrator.h:418-469);
                // VolumePathTracingNEE (:497-581)
                o = xyz(P.ray_o[s]);
                d = xyz(P.ray_d[s]);
                bool walk = false;
                float mt = 0.0f, mt1 = 0.0f;
                v3 tt = mk(1, 1, 1), sa = mk(0, 0, 0);
                if (INTEG == XRT_INTEGRATOR_VPT_NEE && (st & ST_NEEWALK)) {
                    // suspended NEE ratio tracking; the path ray after the scatter is stored
                    if (nee_resume(P, s, thr, rad, rng, g) == 0) {
                        st &= ~ST_NEEWALK;
                        if (depth < P.max_depth) st |= ST_RAY;
                        else finalize = true;
                    }
                } else if (st & ST_MEDIUM) {
                    st &= ~ST_MEDIUM;
                    const f4 m1 = P.med[s], m2 = P.med2[s];
                    mt = m1.x, mt1 = m1.y, sa = mk(m1.z, m1.w, m2.w), tt = xyz(m2);
                    walk = true;
                } else {
                    st &= ~ST_RAY;
                    ++nseg;
                    Surf S;
                    float t1;
                    const f4 h = P.hit[s];
                    const int obj = surface<SCN>(P, s, o, d, h, S, t1);
                    if (obj < 0) {
                        rad = rad + (thr * mk(0.0f, 0.0f, 0.0f)) * (float)(depth != 0);
                        finalize = true;
                    } else {
                        bool alive = true;
                        // russian_roulette (path_common.h), open-coded here and below: the call lowers occupancy
                        if (depth > 0) {
                            const float p = smin((thr.x + thr.y + thr.z) / 3.0f, 1.0f);
                            if (rng.next() >= p) alive = false, finalize = true;
                            else thr = thr / mk(p, p, p);
                        }
                        const DObj ob = P.objs[obj];
                        if (alive && ob.light >= 0) {
                            if (INTEG == XRT_INTEGRATOR_VPT || depth == 0)
                                rad = rad + thr * light_Le(P.lights[ob.light], S.ns, d);
                            alive = false, finalize = true;
                        }
                        if (alive) {
                            if (ob.medium >= 0) {
                                // sampleMedium entry (Src/medium.cpp:47-52): t = info.t
                                mt = h.x, mt1 = t1;
                                if (P.medium.kind == XRT_MEDIUM_HETEROGENEOUS)
                                    sa = ld3(P.medium.absorption) * medium_density(P.medium, ray_at(o, d, mt));
                                walk = true;
                            } else {
                                // neither light nor medium: the reference never advances this
                                // ray (endless loop); stop the path and count it.
                                ++nstall;
                                finalize = true;
                            }
                        }
                    }
                }
                if (walk) {
                    v3 pos, dir, tm;
                    const int r = P.medium.kind == XRT_MEDIUM_HETEROGENEOUS
                                      ? delta_track(P, o, d, thr, mt, mt1, tt, sa, rng, g, pos, dir, tm)
                                      : homog_track(P, o, d, thr, mt, mt1, rng, pos, dir, tm);
                    if (r == 2) {
                        st |= ST_MEDIUM;
                        P.med[s] = make_float4(mt, mt1, sa.x, sa.y);
                        P.med2[s] = make_float4(tt.x, tt.y, tt.z, sa.z);
                    } else {
                        int nr = 0;
                        if (INTEG == XRT_INTEGRATOR_VPT_NEE && r == 1) {
                            LScene Lg;   // the scene in global memory (linear scans, SCN_MIXED)
                            Lg.tri = P.tri, Lg.tng = P.tri_ng, Lg.nrm = P.tri_nrm, Lg.box = P.obj_box;
                            Lg.sph = P.sph, Lg.sobj = P.sph_obj, Lg.bx = P.box, Lg.obj = P.objs, Lg.light = P.lights;
                            nr = nee_medium<SCN>(P, Lg, s, pos, d, thr * tm, rad, rng, g, nsh);
                        }
                        o = pos;
                        d = dir;
                        thr = thr * tm;
                        if (r == 1) ++depth;
                        if (nr == 2) {
                            st |= ST_NEEWALK;   // resumes after the refill
                            P.ray_o[s] = pk(o);
                            P.ray_d[s] = pk(d);
                        } else if (depth < P.max_depth) {
                            st |= ST_RAY;
                            P.ray_o[s] = pk(o);
                            P.ray_d[s] = pk(d);
                        } else {
                            finalize = true;
                        }
                    }
                }
            } else if (st & ST_RAY) {
                st &= ~ST_RAY;
                ++nseg;
                o = xyz(P.ray_o[s]);
                d = xyz(P.ray_d[s]);
                Surf S;
                float t1;
                const int obj = surface<SCN>(P, s, o, d, P.hit[s], S, t1);
                if (INTEG == XRT_INTEGRATOR_DIRECT) {
                    // DirectIntegrator::integrate (Src/integrator.h:82-119)
                    if (obj < 0) {
                        rad = mk((float)0.18, (float)0.18, (float)0.18);
                        finalize = true;
                    } else if (P.objs[obj].light >= 0) {
                        rad = light_Le(P.lights[P.objs[obj].light], S.ns, d);
                        finalize = true;
                    } else {
                        const DObj ob = P.objs[obj];
                        uint32_t smask = 0;
                        for (int l = 0; l < P.n_lights; ++l) {
                            v3 wi = mk(0, 0, 0);
                            float tmax = 0.0f, pdf = 0.0f;
                            const v3 L = light_sample(P.lights[l], S.pos, wi, pdf, tmax, rng);
                            if (pdf == 0.0f) continue;
                            const float bias = 0.01f;
                            const float cosv = smax(0.0f, dot(S.ng, wi));
                            const v3 fr = eval_bxdf(ob);
                            P.sh_o[(size_t)l * P.n_slots + s] = pk(S.pos + S.ng * bias, tmax - bias);
                            P.sh_d[(size_t)l * P.n_slots + s] = pk(wi);
                            P.sh_c[(size_t)l * P.n_slots + s] = pk(((fr * L) * cosv) / pdf);
                            smask |= 1u << l;
                            ++nsh;
                        }
                        if (smask) st |= ST_NEE | ST_END | (smask << ST_SHADOW_SHIFT);
                        else finalize = true;
                    }
                } else if (INTEG == XRT_INTEGRATOR_NORMAL) {
                    // NormalIntegrator::integrate (Src/integrator.h:28-37): 0.5 * (ns + 1)
                    if (obj >= 0) rad = normal_color(S.ns);
                    finalize = true;
                } else {
                    // GIIntegrator::integrate loop body (Src/integrator.h:214-284);
                    // IndirectIntegrator (Src/integrator.h:138-185): no light sampling, Le at
                    // every depth
                    if (obj < 0) {
                        rad = rad + thr * mk(0.0f, 0.0f, 0.0f);
                        finalize = true;
                    } else {
                        bool alive = true;
                        if (depth > 0) {
                            const float p = smin((thr.x + thr.y + thr.z) / 3.0f, 1.0f);
                            if (rng.next() >= p) alive = false, finalize = true;
                            else thr = thr / mk(p, p, p);
                        }
                        const DObj ob = P.objs[obj];
                        if (alive && ob.light >= 0) {
                            if (depth == 0 || INTEG == XRT_INTEGRATOR_INDIRECT)
                                rad = rad + thr * light_Le(P.lights[ob.light], S.ns, d);
                            alive = false, finalize = true;
                        }
                        if (alive) {
                            uint32_t smask = 0;
                            for (int l = 0; l < (INTEG == XRT_INTEGRATOR_GI ? P.n_lights : 0); ++l) {
                                v3 wi = mk(0, 0, 0);
                                float tmax = 0.0f, pdf = 0.0f;
                                const v3 L = light_sample(P.lights[l], S.pos, wi, pdf, tmax, rng);
                                if (pdf == 0.0f) continue;
                                const float bias = 0.01f;
                                const float cosv = smax(0.0f, dot(S.ng, wi));
                                const v3 fr = eval_bxdf(ob);
                                P.sh_o[(size_t)l * P.n_slots + s] = pk(S.pos + S.ng * bias, tmax - bias);
                                P.sh_d[(size_t)l * P.n_slots + s] = pk(wi);
                                P.sh_c[(size_t)l * P.n_slots + s] = pk(((fr * L) * cosv) / pdf);
                                smask |= 1u << l;
                                ++nsh;
                            }
                            if (smask) {
                                P.thr_prev[s] = pk(thr);
                                st |= ST_NEE | (smask << ST_SHADOW_SHIFT);
                            } else if (INTEG == XRT_INTEGRATOR_GI) {
                                rad = rad + thr * mk(0, 0, 0);   // radiance += thr * directL(=0)
                            }
                            lambert_bounce(ob, S, rng, thr, o, d);   // indirect light
                            ++depth;
                            if (depth < P.max_depth) {
                                st |= ST_RAY;
                                P.ray_o[s] = pk(o);
                                P.ray_d[s] = pk(d);
                            } else if (smask) {
                                st |= ST_END;
                            } else {
                                finalize = true;
                            }
                        }
                    }
                }
            }

            // ---- 3. finish the sample, start the next one (Src/renderer.cpp:42-76)
            while (finalize) {
                finalize = false;
                if (st & ST_REGEN) {
                    st &= ~ST_REGEN;
                } else {
                    const v3 r = rad / 1.0f;   // integrate(...) / pdf, pdf = 1
                    if (radiance_invalid(r)) {
                        ++nrej;
                    } else {
                        const SlotPixel pix = slot_pixel_rowmajor(P, s);
                        const uint32_t col = pix.col, row = pix.row;
                        float* px = P.fb + 3 * ((size_t)col + (size_t)P.width * row);
                        px[0] = px[0] + r.x, px[1] = px[1] + r.y, px[2] = px[2] + r.z;
                        if (MOM) {   // s1 = s1 + l, s2 = s2 + l * l (include/xrt.h, xrt_render_var)
                            const float l = luminance(r);
                            float2 m = mom[s];
                            m.x = m.x + l, m.y = m.y + l * l;
                            mom[s] = m;
                        }
                    }
                    ++k;
                }
                st &= ~(ST_END | ST_RAY);
                if (k >= P.spp) {
                    st = ST_DONE;
                    break;
                }
                // regenerate: jitter draws, camera ray (sample_start, path_common.h, open-coded here
                // and below: the call adds SGPR spills)
                const SlotPixel pix = slot_pixel_rowmajor(P, s);
                const uint32_t col = pix.col, row = pix.row;
                const float u = div_w(P, (float)(int)col + rng.next());
                const float v = div_h(P, (float)(int)row + rng.next());
                camera_ray(P, u, v, o, d);
                thr = mk(1, 1, 1);
                rad = mk(0, 0, 0);
                depth = 0;
                if (!one_hit(INTEG) && P.max_depth == 0) {
                    finalize = true;   // the bounce loop never runs: radiance 0
                    continue;
                }
                st |= ST_RAY;
                P.ray_o[s] = pk(o);
                P.ray_d[s] = pk(d);
            }
            if (st & ST_REGEN) {   // very first sample of the slot
                st &= ~ST_REGEN;
                // a progressive session's passes each start here; its records were zeroed once, by begin
                if (MOM && !(P.rflags & kRflagSession)) mom[s] = make_float2(0.0f, 0.0f);
                const SlotPixel pix = slot_pixel_rowmajor(P, s);
                const uint32_t col = pix.col, row = pix.row;
                const float u = div_w(P, (float)(int)col + rng.next());
                const float v = div_h(P, (float)(int)row + rng.next());
                camera_ray(P, u, v, o, d);
                thr = mk(1, 1, 1);
                rad = mk(0, 0, 0);
                depth = 0;
                if (!one_hit(INTEG) && P.max_depth == 0) {
                    // degenerate: every sample is 0 — finish all of them here
                    while (true) {
                        ++k;
                        if (k >= P.spp) { st = ST_DONE; break; }
                        (void)rng.next(), (void)rng.next();
                    }
                } else {
                    st |= ST_RAY;
                    P.ray_o[s] = pk(o);
                    P.ray_d[s] = pk(d);
                }
            }
            P.state[s] = st;
            P.depth[s] = depth;
            P.sample_k[s] = k;
            P.thr[s] = pk(thr);
            P.rad[s] = pk(rad);
            P.rng_c[s] = rng.c;
            if (nseg) P.c_seg[s] += nseg;
            if (nsh) P.c_shadow[s] += nsh;
            if (nrej) P.c_rej[s] += nrej;
            if (nstall) P.c_stall[s] += nstall;
        }
        // ---- 4. compaction (ballot + prefix count, one atomic per wave), then the wave's
        // refills in-line, overlapping other waves' shading instead of a serial k_refill
        wave_append(valid && !(st & ST_DONE), s, out + it.p * P.part_cap, out_count + it.p, lane);
        wave_refill(P, want_req && !(st & ST_DONE), s, g, lane, rbuf[tid >> 6]);
    }
    (void)req_count_or_mom;
}

hipError_t launch_shade(const KParams& P, const uint32_t* list, const uint32_t* count, uint32_t* out,
                        uint32_t* out_count, uint32_t* req_count, uint32_t blocks, hipStream_t st, float2* mom) {
    return with_scene_kind(P.scene_kind, [&](auto scn) {
        return with_integrator(P.integrator, [&](auto integ) {
            if (mom)
                hipLaunchKernelGGL((k_shade<decltype(scn)::value, decltype(integ)::value, true>), dim3(blocks), dim3(kBlock),
                                   0, st, P, list, count, out, out_count, mom);
            else
                hipLaunchKernelGGL((k_shade<decltype(scn)::value, decltype(integ)::value>), dim3(blocks), dim3(kBlock), 0,
                                   st, P, list, count, out, out_count, req_count);
            return hipGetLastError();
        });
    });
}

}  // namespace xrt
