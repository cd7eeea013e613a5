// medium.h — participating media for the volumetric integrators (k_shade in shade.hip, k_step
// in step.hip): the density grid lookup, the wavelength and phase-function samplers, delta /
// ratio tracking, the homogeneous media, and VolumePathTracingNEE's light sample.
#pragma once
#include "lscene.h"
#include "path_common.h"

namespace xrt {

// ==================================================================== medium ====
// DensityGrid::getDensity = OpenVDB BoxSampler::wsSample (Src/grid.h:71-77): index-space
// position in double, floor, trilinear lerps a + float((b - a) * w) (z, then y, then x),
// background 0 outside the voxels.
__device__ __forceinline__ float grid_value(const DMedium& M, int i, int j, int k) {
    if (i < 0 || j < 0 || k < 0 || i >= M.nx || j >= M.ny || k >= M.nz) return 0.0f;
    return M.density[((size_t)k * M.ny + (size_t)j) * M.nx + (size_t)i];
}
__device__ __forceinline__ float vdb_lerp(float a, float b, double w) { return a + (float)((double)(b - a) * w); }
// sparse leaf bricks: one voxel (background 0 outside the grid and in inactive bricks)
__device__ __forceinline__ float brick_value(const DMedium& M, int i, int j, int k) {
    if (i < 0 || j < 0 || k < 0 || i >= M.nx || j >= M.ny || k >= M.nz) return 0.0f;
    const int b = M.brick_table[((k >> 3) * M.nby + (j >> 3)) * M.nbx + (i >> 3)];
    return b < 0 ? 0.0f : M.bricks[(size_t)b * 512 + (((k & 7) * 8 + (j & 7)) * 8 + (i & 7))];
}
// OpenVDB BoxSampler cell of a world position: index-space coordinates in double, the
// lower corner (i, j, k) and the fractional weights
struct VdbCell {
    double u, v, w;
    int i, j, k;
};
__device__ __forceinline__ VdbCell vdb_cell(const DMedium& M, v3 p) {
    const double inv = M.inv_voxel;
    const double xi = ((double)p.x - (double)M.origin[0]) * inv;
    const double yi = ((double)p.y - (double)M.origin[1]) * inv;
    const double zi = ((double)p.z - (double)M.origin[2]) * inv;
    const double fx = __builtin_floor(xi), fy = __builtin_floor(yi), fz = __builtin_floor(zi);
    VdbCell C;
    C.i = (int)fx, C.j = (int)fy, C.k = (int)fz;
    C.u = xi - fx, C.v = yi - fy, C.w = zi - fz;
    return C;
}
// dense grid, all eight corners inside: the x-neighbours are adjacent words, four dword-aligned
// dwordx2 loads, corners in the order d000 d001 d010 d011 d100 d101 d110 d111
__device__ __forceinline__ bool dense_interior(const DMedium& M, const VdbCell& C) {
    return !M.brick_table && C.i >= 0 && C.j >= 0 && C.k >= 0 && C.i + 1 < M.nx && C.j + 1 < M.ny && C.k + 1 < M.nz;
}
__device__ __forceinline__ void dense_corners(const DMedium& M, const VdbCell& C, float (&q)[8]) {
    if (M.corners) {
        const f4* r = reinterpret_cast<const f4*>(M.corners) +
                      2 * (((size_t)C.k * (M.ny - 1) + (size_t)C.j) * (M.nx - 1) + (size_t)C.i);
        const f4 a = r[0], b = r[1];
        q[0] = a.x, q[1] = a.y, q[2] = a.z, q[3] = a.w, q[4] = b.x, q[5] = b.y, q[6] = b.z, q[7] = b.w;
        return;
    }
    typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
    using g2 = __attribute__((address_space(1))) const f2u;
    const float* b = M.density + ((size_t)C.k * M.ny + (size_t)C.j) * M.nx + (size_t)C.i;
    const size_t sy = (size_t)M.nx, sz = (size_t)M.nx * M.ny;
    const f2u a = *(g2*)b, c = *(g2*)(b + sz), e = *(g2*)(b + sy), f = *(g2*)(b + sy + sz);
    q[0] = a.x, q[4] = a.y, q[1] = c.x, q[5] = c.y, q[2] = e.x, q[6] = e.y, q[3] = f.x, q[7] = f.y;
}
__device__ __forceinline__ float vdb_interp(const DMedium& M, const VdbCell& C, const float (&q)[8]) {
    const float g = vdb_lerp(vdb_lerp(vdb_lerp(q[0], q[1], C.w), vdb_lerp(q[2], q[3], C.w), C.v),
                             vdb_lerp(vdb_lerp(q[4], q[5], C.w), vdb_lerp(q[6], q[7], C.w), C.v), C.u);
    return M.multiplier * g;   // HeterogeneousMedium::getDensity (Src/medium.cpp:24-27)
}

static __device__ float medium_density(const DMedium& M, v3 p) {
    const VdbCell C = vdb_cell(M, p);
    const int i = C.i, j = C.j, k = C.k;
    float q[8];
    if (M.brick_table) {
        // a cell inside one brick: one table lookup, x-neighbours adjacent in the brick
        if (i >= 0 && j >= 0 && k >= 0 && i + 1 < M.nx && j + 1 < M.ny && k + 1 < M.nz && (i & 7) != 7 &&
            (j & 7) != 7 && (k & 7) != 7) {
            const int b = M.brick_table[((k >> 3) * M.nby + (j >> 3)) * M.nbx + (i >> 3)];
            if (b < 0) {
                for (int c = 0; c < 8; ++c) q[c] = 0.0f;
            } else {
                const float* r = M.bricks + (size_t)b * 512 + (((k & 7) * 8 + (j & 7)) * 8 + (i & 7));
                q[0] = r[0], q[4] = r[1], q[2] = r[8], q[6] = r[9];
                q[1] = r[64], q[5] = r[65], q[3] = r[72], q[7] = r[73];
            }
        } else {
            q[0] = brick_value(M, i, j, k), q[1] = brick_value(M, i, j, k + 1);
            q[2] = brick_value(M, i, j + 1, k), q[3] = brick_value(M, i, j + 1, k + 1);
            q[4] = brick_value(M, i + 1, j, k), q[5] = brick_value(M, i + 1, j, k + 1);
            q[6] = brick_value(M, i + 1, j + 1, k), q[7] = brick_value(M, i + 1, j + 1, k + 1);
        }
    } else if (dense_interior(M, C)) {
        dense_corners(M, C, q);
    } else {
        q[0] = grid_value(M, i, j, k), q[1] = grid_value(M, i, j, k + 1);
        q[2] = grid_value(M, i, j + 1, k), q[3] = grid_value(M, i, j + 1, k + 1);
        q[4] = grid_value(M, i + 1, j, k), q[5] = grid_value(M, i + 1, j, k + 1);
        q[6] = grid_value(M, i + 1, j + 1, k), q[7] = grid_value(M, i + 1, j + 1, k + 1);
    }
    return vdb_interp(M, C, q);
}

// Medium::sampleWavelength + DiscreteEmpiricalDistribution1D (Src/medium.h:102-115,
// Src/sampler.h:53-94).  lower_bound past the end is UB in the reference; clamped to 2.
__device__ __forceinline__ uint32_t sample_wavelength(v3 thr, v3 albedo, Rng& rng, v3& pmf) {
    const v3 ta = thr * albedo;
    const float sum = ((0.0f + ta.x) + ta.y) + ta.z;
    const v3 q = div3s(ta, sum);   // ta.x / sum, ta.y / sum, ta.z / sum
    const float c1 = 0.0f + q.x;
    const float c2 = c1 + q.y;
    const float c3 = c2 + q.z;
    pmf = mk(c1 - 0.0f, c2 - c1, c3 - c2);
    const float u = rng.next();
    int x = 0;
    if (0.0f < u) {
        x = 1;
        if (c1 < u) {
            x = 2;
            if (c2 < u) x = (c3 < u) ? 4 : 3;
        }
    }
    if (x == 0) x = 1;
    if (x == 4) x = 3;
    return (uint32_t)(x - 1);
}

// HenyeyGreenstein::sampleDirection (Src/medium.h:37-67); getNext2D = (2nd, 1st draw)
static __device__ void hg_sample(float g, v3 wo, Rng& rng, v3& wi) {
    const float d1 = rng.next();
    const float d2 = rng.next();
    const float u0 = d2, u1 = d1;
    float cosTheta;
    if (__builtin_fabs((double)g) < 1e-3) {
        cosTheta = 2.0f * u0 - 1.0f;
    } else {
        const float sqrTerm = (1.0f - g * g) / (1.0f - g + 2.0f * g * u0);
        cosTheta = (1.0f + g * g - sqrTerm * sqrTerm) / (2.0f * g);
    }
    const float sinTheta = __builtin_sqrtf(smax(1.0f - cosTheta * cosTheta, 0.0f));
    const float phi = 2.0f * kPI * u1;
    float sphi, cphi;
    glibc_sincosf(phi, sphi, cphi);
    const v3 wl = mk(cphi * sinTheta, cosTheta, sphi * sinTheta);
    v3 t, b;
    onb(wo, t, b);
    wi = local_to_world(wl, t, wo, b);
}

__device__ __forceinline__ v3 vexp(v3 a) { return mk(glibc_expf(a.x), glibc_expf(a.y), glibc_expf(a.z)); }
__device__ __forceinline__ bool isnan3(v3 a) {
    return __builtin_isnan(a.x) || __builtin_isnan(a.y) || __builtin_isnan(a.z);
}

// HeterogeneousMedium::sampleMedium — delta tracking with spectral MIS (Src/medium.cpp:
// 45-133), one collision per call: returns 0 = left the medium, 1 = real scattering,
// 2 = suspended because fewer than 8 RNG words remain (the slot resumes after the next
// refill), 3 = null collision (call again).  `t`, `tt` (throughput_tracking) and `sa`
// (sigma_a) carry the loop state.
__device__ __forceinline__ int delta_step(const KParams& P, v3 o, v3 d, v3 thr, float& t, float t1, v3& tt, v3& sa,
                                          Rng& rng, uint32_t g, v3& pos, v3& dir, v3& tm) {
    const DMedium& M = P.medium;
    const float majorant = M.majorant, invMajorant = M.inv_majorant;
    const v3 vmaj = mk(majorant, majorant, majorant);
    const v3 absorb = ld3(M.absorption), scatter = ld3(M.scattering);
    if (g - rng.c < 8u) return 2;
    v3 pmf;
    const uint32_t channel = sample_wavelength(thr * tt, (vmaj - sa) * invMajorant, rng, pmf);
    const float s = -glibc_logf(smax(1.0f - rng.next(), 0.0f)) * invMajorant;
    t += s;
    // the three outcomes share the transmittance and the throughput update: one expf and
    // one quotient per collision however the wave's lanes split (same operands per lane)
    int r = 0;
    float x, fe = 1.0f;   // the expf argument's distance; the majorant factor of the pdf
    v3 num = mk(0, 0, 0), Px = mk(1, 1, 1);
    if (t > t1 - kRAY_EPS) {
        pos = ray_at(o, d, t1 + kRAY_EPS);
        dir = d;
        x = s - (t - (t1 - kRAY_EPS));
    } else {
        const float density = medium_density(M, ray_at(o, d, t));
        const v3 sigma_s = scatter * density;
        sa = absorb * density;
        const v3 sigma_n = (vmaj - sa) - sigma_s;
        const v3 den = sigma_s + sigma_n;
        x = s, fe = majorant;
        // P_s = sigma_s / (sigma_s + sigma_n): the acceptance test reads one component
        r = rng.next() < comp(sigma_s, channel) / comp(den, channel) ? 1 : 3;
        if (r == 1) {
            pos = ray_at(o, d, t);
            hg_sample(M.g, d, rng, dir);
        }
        num = r == 1 ? sigma_s : sigma_n;
        Px = div3v(num, den);
    }
    const float e = glibc_expf(-majorant * x);   // vexp((-vmaj) * x): three equal arguments
    const v3 tr = mk(e, e, e);
    const v3 pdf = r == 0 ? pmf * tr : (pmf * (tr * fe)) * Px;
    tt = tt * div3s(r == 0 ? tr : tr * num, pdf.x + pdf.y + pdf.z);
    if (r != 3) tm = isnan3(tt) ? mk(0, 0, 0) : tt;
    return r;
}
// the whole walk (0, 1 or 2 as delta_step)
static __device__ int delta_track(const KParams& P, v3 o, v3 d, v3 thr, float& t, float t1, v3& tt, v3& sa, Rng& rng,
                           uint32_t g, v3& pos, v3& dir, v3& tm) {
    for (;;) {
        const int r = delta_step(P, o, d, thr, t, t1, tt, sa, rng, g, pos, dir, tm);
        if (r != 3) return r;
    }
}

// HenyeyGreenstein::evaluate (Src/medium.h:29-34)
__device__ __forceinline__ float hg_eval(float g, v3 wo, v3 wi) {
    const float cosTheta = dot(wo, wi);
    const float denom = 1.0f + g * g - 2.0f * g * cosTheta;
    return kPI_MUL_4_INV * (1.0f - g * g) / (denom * __builtin_sqrtf(denom));
}

// HeterogeneousMedium::ratioTrackingTransmittance (Src/medium.h:360-386), resumable like
// delta_track: false = suspended (fewer than 8 RNG words left); `t`, `tr` carry the loop.
static __device__ bool ratio_track(const KParams& P, v3 p1, v3 dn, float dist, float& t, v3& tr, Rng& rng, uint32_t g) {
    const DMedium& M = P.medium;
    const float majorant = M.majorant, invMajorant = M.inv_majorant;
    const v3 vmaj = mk(majorant, majorant, majorant);
    const v3 absorb = ld3(M.absorption), scatter = ld3(M.scattering);
    for (;;) {
        if (g - rng.c < 8u) return false;
        const float s = -glibc_logf(smax(1.0f - rng.next(), 0.0f)) * invMajorant;
        t += s;
        if (t > dist) return true;
        const float density = medium_density(M, ray_at(p1, dn, t));
        const v3 sigma_n = (vmaj - absorb * density) - scatter * density;
        tr = tr * (sigma_n * invMajorant);
    }
}

// Homogeneous media (Src/medium.h:122-277): one free-flight sample per visit of the medium
// box, analytic transmittance exp(-sigma_t * t) (Medium::analyticTransmittance).  Same
// return contract as delta_track (0 = left the medium, 1 = scattering); never suspends
// (at most 4 draws).  t, t1: the box hit's entry / exit (IntersectInfo t, t1).
__device__ __forceinline__ v3 analytic_tr(float t, v3 sigma_t) { return vexp((-sigma_t) * t); }
static __device__ int homog_track(const KParams& P, v3 o, v3 d, v3 thr, float t0, float t1, Rng& rng, v3& pos, v3& dir,
                           v3& tm) {
    const DMedium& M = P.medium;
    const v3 ss = ld3(M.scattering), st = ld3(M.sigma_t);
    const float distToSurface = t1 - t0;
    if (M.kind == XRT_MEDIUM_HOMOGENEOUS_MIS) {
        // HomogeneousMediumMIS::sampleMedium (Src/medium.h:154-191)
        v3 pmf;
        const uint32_t channel = sample_wavelength(thr, div3v(ss, st), rng, pmf);
        const float t = -glibc_logf(smax(1.0f - rng.next(), 0.0f)) / comp(st, channel);
        if (t > distToSurface - kRAY_EPS) {
            pos = ray_at(o, d, t1 + kRAY_EPS);
            dir = d;
            const v3 tr = analytic_tr(distToSurface, st);
            const v3 pdf = pmf * tr;
            tm = div3s(tr, pdf.x + pdf.y + pdf.z);
            return 0;
        }
        hg_sample(M.g, d, rng, dir);
        pos = ray_at(o, d, t0 + t);
        const v3 tr = analytic_tr(t, st);
        const v3 pdf = pmf * (st * tr);
        tm = div3s(tr * ss, pdf.x + pdf.y + pdf.z);
        return 1;
    }
    if (M.kind == XRT_MEDIUM_HOMOGENEOUS_ACHROMATIC) {
        // HomogeneousMediumAchromatic::sampleMedium (Src/medium.h:201-229)
        const float t = -glibc_logf(smax(1.0f - rng.next(), 0.0f)) / st.x;
        if (t > distToSurface - kRAY_EPS) {
            pos = ray_at(o, d, t1 + kRAY_EPS);
            dir = d;
            tm = mk(1.0f, 1.0f, 1.0f);
            return 0;
        }
        hg_sample(M.g, d, rng, dir);
        pos = ray_at(o, d, t0 + t);
        tm = div3v(ss, st);
        return 1;
    }
    // HomogeneousMediumNoMIS::sampleMedium (Src/medium.h:240-275)
    int channel = (int)(3.0f * rng.next());
    if (channel == 3) channel--;
    const float pmf_wavelength = 1.0f / 3.0f;
    const float sc = comp(st, (uint32_t)channel);
    const float t = -glibc_logf(smax(1.0f - rng.next(), 0.0f)) / sc;
    const float pdf_distance = sc * glibc_expf(-sc * t);
    if (t > distToSurface - kRAY_EPS) {
        pos = ray_at(o, d, t1 + kRAY_EPS);
        dir = d;
        const v3 tr = analytic_tr(distToSurface, st);
        const float p_surface = glibc_expf(-sc * distToSurface);
        tm = (tr * (1.0f / 3.0f)) / (pmf_wavelength * p_surface);
        return 0;
    }
    hg_sample(M.g, d, rng, dir);
    pos = ray_at(o, d, t0 + t);
    tm = ((analytic_tr(t, st) * (1.0f / 3.0f)) * ss) / (pmf_wavelength * pdf_distance);
    return 1;
}

// VolumePathTracingNEE's light sample at a scattering point (Src/integrator.h:539-560):
// sampleDirectionToLight (:586-602, Scene::sampleAreaLight Src/scene.cpp:182-188) and
// isVisible (:604-631) — the shadow ray's closest hit; a surface occludes, a medium
// attenuates by ratio tracking between the hit's t and t1.  Adds
// (thr * tm) * (transmittance * f * Le / pdf) to rad and returns 0, or returns 2 with the
// ratio tracking suspended (state in P.nee, resumed by nee_resume).  Media make a scene
// SCN_MIXED, so other scene kinds never get here.
template <int SCN>
__device__ int nee_medium(const KParams& P, const LScene& L, uint32_t s, v3 pos, v3 wo, v3 thr_m, v3& rad, Rng& rng,
                          uint32_t g, uint32_t& nsh) {
    if (SCN != SCN_MIXED) return 0;
    uint32_t li = (uint32_t)((float)P.n_lights * rng.next());   // size() * getNext1D(), truncated
    if (li == (uint32_t)P.n_lights) li--;
    const float choose = 1.0f / (float)P.n_lights;
    v3 wl = mk(0, 0, 0);
    float lpdf = 0.0f, dist = 0.0f;
    const v3 Le = light_sample(L.light[li], pos, wl, lpdf, dist, rng);
    const float pdf_dir = choose * lpdf;
    if (!(pdf_dir > 0.0f)) return 0;
    ++nsh;
    HitRec h;
    closest_l<SCN>(P, L, pos, wl, h);
    v3 tr = mk(1, 1, 1);
    const float f = hg_eval(P.medium.g, wo, wl);
    if (h.code >= 0) {
        const DObj ob = L.obj[hit_object(L, h)];
        if (ob.material != XRT_MAT_NONE) return 0;   // hasSurface(): occluded
        if (ob.medium >= 0 && P.medium.kind != XRT_MEDIUM_HETEROGENEOUS) {
            // HomogeneousMedium::transmittance (Src/medium.h:133-137)
            const v3 p1 = ray_at(pos, wl, h.t), p2 = ray_at(pos, wl, h.t1);
            tr = tr * analytic_tr(length(p1 - p2), ld3(P.medium.sigma_t));
        } else if (ob.medium >= 0) {
            const v3 p1 = ray_at(pos, wl, h.t), p2 = ray_at(pos, wl, h.t1);
            const float dist_end = length(p1 - p2);
            const v3 dn = normalize(p2 - p1);
            float t = 0.0f;
            if (!ratio_track(P, p1, dn, dist_end, t, tr, rng, g)) {
                const size_t n = P.n_slots;
                P.nee[s] = make_float4(p1.x, p1.y, p1.z, t);
                P.nee[n + s] = make_float4(dn.x, dn.y, dn.z, dist_end);
                P.nee[2 * n + s] = make_float4(tr.x, tr.y, tr.z, f);
                P.nee[3 * n + s] = make_float4(Le.x, Le.y, Le.z, pdf_dir);
                return 2;
            }
        }
    }
    rad = rad + thr_m * (((tr * f) * Le) / pdf_dir);
    return 0;
}

// resume a suspended NEE ratio tracking; thr_m = the path throughput after the scatter
static __device__ int nee_resume(const KParams& P, uint32_t s, v3 thr_m, v3& rad, Rng& rng, uint32_t g) {
    const size_t n = P.n_slots;
    const f4 a = P.nee[s], b = P.nee[n + s], c = P.nee[2 * n + s], d = P.nee[3 * n + s];
    float t = a.w;
    v3 tr = xyz(c);
    if (!ratio_track(P, xyz(a), xyz(b), b.w, t, tr, rng, g)) {
        P.nee[s] = make_float4(a.x, a.y, a.z, t);
        P.nee[2 * n + s] = make_float4(tr.x, tr.y, tr.z, c.w);
        return 2;
    }
    rad = rad + thr_m * (((tr * c.w) * xyz(d)) / d.w);
    return 0;
}

}  // namespace xrt
