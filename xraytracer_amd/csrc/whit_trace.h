// whit_trace.h — the trace policies and LDS carves of the one-wave-per-pixel kernels that run
// over any scene the Whitted schedules hold: whitted.hip (k_whitted, k_whitted_bvh) and aov.hip
// (k_aov, k_aov_bvh).  A policy has three members — closest (Scene::intersect into a HitRec),
// occluded (Scene::occluded) and surface (the hit's SurfaceInfo; returns the object index,
// -1 = miss) — and `obj`, the object table that index goes into.
//   WhitLds, whit_wave_off                   : a scene resident in LDS (k_whitted, k_aov)
//   WhitBvhLayout, WhitBvh                   : a triangle scene beyond LDS through its BVH
//   whit_bvh_setup, with_whit_bvh            : the block setup and the host dispatch of the two
//                                              kernels over WhitBvh (k_whitted_bvh, k_aov_bvh)
// The BVH's own share of LDS (top nodes, stack entry size) is bvh_walk.h's BvhLds.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bvh_walk.h"
#include "lds_stream.h"
#include "lscene.h"
#include "path_common.h"

namespace xrt {

constexpr int kWhitBlock = 256;                                       // 4 waves share one LDS scene copy
constexpr uint32_t kWhitWaveLds = (kMT + 3 * kPixSumStride) * 4;    // stream + ordered-sum buffer

// WhitLds: the LDS-resident scene (lscene.h), whatever its kind.
template <int SCN>
struct WhitLds {
    const KParams& P;
    const LScene& L;
    const DObj* obj;
    __device__ __forceinline__ void closest(v3 o, v3 d, HitRec& h) const { closest_l<SCN>(P, L, o, d, h); }
    __device__ __forceinline__ bool occluded(v3 o, v3 d, float tmax) const { return occluded_l<SCN>(P, L, o, d, tmax); }
    __device__ __forceinline__ int surface(v3 o, v3 d, const HitRec& h, Surf& S) const {
        return surface_l<SCN>(L, o, d, h, S);
    }
};

// LDS bytes: the scene carve (step_layout), then one stream + sum slice per wave
__host__ __device__ inline uint32_t whit_wave_off(const KParams& P) { return (step_layout(P).total + 15u) & ~15u; }

// WhitBvh: a triangle scene beyond LDS through its triangle BVH (whitted.hip describes the
// three accessors).  The traversal stack (P.bvh_stack entries per thread, 16-bit when the node
// indices fit) and the top of the tree are in LDS as in k_trace_bvh.
struct WhitBvhLayout {
    uint32_t tri, box, plane, stack, wave, total;   // bytes; the top nodes are at 0
};
__host__ __device__ inline WhitBvhLayout whit_bvh_layout(const KParams& P) {
    const BvhLds B = bvh_lds(P);
    const uint32_t nt = P.two_level ? (uint32_t)P.n_stri : 0u, ns = P.two_level ? (uint32_t)P.n_sobj : 0u;
    WhitBvhLayout L;
    L.tri = B.stack();
    L.box = L.tri + 48u * nt;
    L.plane = L.box + (uint32_t)sizeof(DObjBox) * ns;
    L.stack = (L.plane + (uint32_t)sizeof(DObjPlane) * ns + 15u) & ~15u;
    L.wave = (L.stack + (uint32_t)P.bvh_stack * kWhitBlock * B.entry + 15u) & ~15u;
    L.total = L.wave + (kWhitBlock / 64) * kWhitWaveLds;
    return L;
}

template <bool TWO, typename SE>
struct WhitBvh {
    const KParams& P;
    const f4* top;   // the first ntop nodes (LDS); top[0..3] is the root
    int ntop;
    SE* stk;         // this thread's stack, entries kWhitBlock apart
    const f4* ltri;  // two-level: the small objects' triangles, boxes and planes (LDS)
    const DObjBox* lbox;
    const DObjPlane* lpl;
    const DObj* obj;
    __device__ __forceinline__ void closest(v3 o, v3 d, HitRec& h) const {
        h.t = kINF, h.u = h.v = 0.0f, h.code = -1;
        if (TWO) {
            const v3 inv = rcp3(d);
            for (int ob = 0; ob < P.n_sobj; ++ob) {
                const DObjBox B = lbox[ob];
                if (plane_away_w(o, d, lpl[ob]) || !box_overlap(o, inv, B, h.t)) continue;
                const int end = B.first + (B.count_occ & 0x7fffffff);
                for (int k = B.first; k < end; ++k) {
                    const f4 E2 = ltri[3 * k + 2];
                    float t, u, v;
                    if (ray_tri(o, d, xyz(ltri[3 * k]), xyz(ltri[3 * k + 1]), xyz(E2), t, u, v) && t < h.t)
                        h.t = t, h.u = u, h.v = v, h.code = __float_as_int(E2.w);
                }
            }
            if (!root_overlap(top[0], top[1], top[2], top[3], o, inv, h.t)) return;
        }
        (void)bvh_trace<false, SE, kWhitBlock>(P, top, ntop, stk, o, d, kINF, h.t, h.u, h.v, h.code);
    }
    __device__ __forceinline__ bool occluded(v3 o, v3 d, float tmax) const {
        if (TWO) {
            const v3 inv = rcp3(d);
            for (int ob = 0; ob < P.n_sobj; ++ob) {
                const DObjBox B = lbox[ob];
                if (B.count_occ >= 0 || plane_away_w(o, d, lpl[ob]) || !box_overlap(o, inv, B, tmax)) continue;
                const int end = B.first + (B.count_occ & 0x7fffffff);
                for (int k = B.first; k < end; ++k) {
                    float t, u, v;
                    if (ray_tri(o, d, xyz(ltri[3 * k]), xyz(ltri[3 * k + 1]), xyz(ltri[3 * k + 2]), t, u, v) && t < tmax)
                        return true;
                }
            }
            if (!root_overlap(top[0], top[1], top[2], top[3], o, inv, tmax)) return false;
        }
        float bt = kINF, bu = 0.0f, bv = 0.0f;
        int bk = -1;
        return bvh_trace<true, SE, kWhitBlock>(P, top, ntop, stk, o, d, tmax, bt, bu, bv, bk);
    }
    __device__ __forceinline__ int surface(v3 o, v3 d, const HitRec& h, Surf& S) const {
        float t1;
        return xrt::surface<SCN_TRI>(P, 0u, o, d, make_float4(h.t, h.u, h.v, __int_as_float(h.code)), S, t1);
    }
};

// The block's setup of k_whitted_bvh and k_aov_bvh over its dynamic LDS `lb`: carves the layout,
// copies the top nodes and (TWO) the small objects in, syncs the block, and returns the policy
// with the wave's slice (kWhitWaveLds: the stream, then the sum buffer).
template <bool TWO, typename SE>
struct WhitBvhBlock {
    WhitBvh<TWO, SE> T;
    uint32_t* st;
};
template <bool TWO, typename SE>
__device__ __forceinline__ WhitBvhBlock<TWO, SE> whit_bvh_setup(const KParams& P, char* lb, int tid) {
    const WhitBvhLayout Lo = whit_bvh_layout(P);
    const BvhLds B = bvh_lds(P);
    f4* ltri = reinterpret_cast<f4*>(lb + Lo.tri);
    DObjBox* lbox = reinterpret_cast<DObjBox*>(lb + Lo.box);
    DObjPlane* lpl = reinterpret_cast<DObjPlane*>(lb + Lo.plane);
    (void)bvh_top_load<SE>(lb, P.bvh_node, B, tid, kWhitBlock);
    if (TWO) {
        lds_copy(ltri, P.stri, 3 * P.n_stri, tid, kWhitBlock);
        lds_copy(lbox, P.sbox, P.n_sobj, tid, kWhitBlock);
        lds_copy(lpl, P.splane, P.n_sobj, tid, kWhitBlock);
    }
    SE* stk = reinterpret_cast<SE*>(lb + Lo.stack) + tid;
    uint32_t* st = reinterpret_cast<uint32_t*>(lb + Lo.wave + (tid >> 6) * kWhitWaveLds);
    __syncthreads();
    return {{P, reinterpret_cast<const f4*>(lb), B.ntop, stk, ltri, lbox, lpl, P.objs}, st};
}

// fn(std::bool_constant<TWO>{}, SE{}): the build of a WhitBvh kernel for this scene — two-level
// or not, and the stack entry type its tree takes
template <typename F>
auto with_whit_bvh(const KParams& P, F&& fn) {
    return with_stack_entry(bvh_lds(P), [&](auto se) {
        return P.two_level ? fn(std::true_type{}, se) : fn(std::false_type{}, se);
    });
}

}  // namespace xrt
