// wave_deep.h — the two-level trace inside the wave, for the merged step kernels
// (step_merged.h: k_step_merged<..., BVH = true>).  Device code, and the LDS layout both sides use.
//
// The fused schedule for two-level scenes (C4: the Cornell box around a 51,200-triangle
// sphere mesh): after merged_trace (merged.h) has tested the small
// objects (LDS, pair passes, keys (t bits << 32 | original index)), the rays whose segment
// still reaches the BVH — extension rays over [0, best t], shadow rays over [0, tmax] if no
// small object occluded them — are ranked into the wave's scratch and walked by the wave's
// 16 quads, k_trace_deep4q's four-lanes-per-ray walk of the 4-wide BVH (lane c owns child
// c of the current node; the quad shares the pruning limit, occlusion and the next node by
// DPP), a quad taking the next ranked ray when its walk ends.  Results merge into the
// wave's records as merged_trace leaves them: the smallest (t, original index) key by the
// lane holding it, occlusion bits by an or.  Exact for the reasons k_trace_deep4q is (every
// triangle whose padded box overlaps [0, best t] is tested by some lane) — the same
// lexicographic minimum over every triangle the reference's linear scan tests
// (Src/scene.cpp:190-211, Src/primitive.cpp:83-168).
#pragma once
#include "bvh.h"
#include "merged.h"
#include "path_common.h"
#include "trace_common.h"

namespace xrt {

constexpr int kQs = 64;          // quad stack entries (circular; >= kBvh4Stack)
constexpr int kQsMask = kQs - 1;
static_assert(kQs >= kBvh4Stack, "quad stacks");

// The walk of n_deep ranked rays ray_o / ray_d (w: tmax resp. the ray id q * 64 + lane; q = 0:
// extension ray, closest hit from the key best[lane]; 1 + l: shadow ray l, occlusion bit l of
// occ[lane]).  top: the first ntop 4-wide nodes in LDS; stk: this wave's 16 quad stacks
// (stride 16).  Must be called by every lane of the wave.
template <typename SE>
__device__ __forceinline__ void wave_deep_walk(const KParams& P, const f4* top, int ntop, SE* stk, const f4* ray_o,
                                               const f4* ray_d, unsigned long long* best, uint32_t* occ, int lane,
                                               uint32_t n_deep) {
    constexpr uint64_t kLeads = 0x1111111111111111ull;   // lane 0 of every quad
    const int c = lane & 3;
    SE* qs = stk + (lane >> 2);
    uint32_t next = 0;   // wave-uniform: first ray not yet taken
    bool active = false, any = false;
    uint32_t id = 0;   // the ray's id
    int node = 0, sp = 0, base = 0, bk = -1;   // stack entries [base, sp), circular (kQs)
    v3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.0f, bt = kINF;
    while (true) {
        if (next < n_deep) {
            const uint64_t idle = __ballot(!active) & kLeads;
            if (idle) {
                const uint32_t idx = next + (uint32_t)__popcll(idle & ((1ull << (lane & ~3)) - 1ull));
                if (!active && idx < n_deep) {
                    const f4 A = ray_o[idx], D = ray_d[idx];
                    id = __float_as_uint(D.w);
                    any = id >= 64u;
                    o = xyz(A), d = xyz(D), tmax = A.w;
                    bt = kINF, bk = -1;
                    if (!any) {
                        const unsigned long long key = best[id];
                        if (key != ~0ull) bt = __uint_as_float((uint32_t)(key >> 32)), bk = (int)(uint32_t)key;
                    }
                    inv = rcp3(d);
                    node = 0, sp = 0, base = 0;
                    active = true;
                }
                next += (uint32_t)__popcll(idle);
            }
        }
        if (!__ballot(active)) break;
        if (!active) continue;
        // ---- one node, with as few divergent branches as the step allows (the loop's exec-mask
        // bookkeeping cost about as many scalar instructions as it had vector ones): the node
        // from LDS or global memory through one generic pointer, every leaf triangle's test and
        // both reductions computed for closest-hit and any-hit rays alike, the stack top read
        // every step.  (Measured and not kept, DESIGN.md §3: a branchy form, fetching the likely
        // next node before the leaf tests, work stealing between quads.)
        const f4* N = node < ntop ? top + 8 * node : P.bvh4 + 8 * (size_t)node;
        const f4 lo = N[c], hi = N[4 + c];
        const int cidx = __float_as_int(lo.w), ccnt = __float_as_int(hi.w);
        const float lim0 = any ? tmax : __uint_as_float(group_min32<4>(__float_as_uint(bt)));   // t >= 0: bits order
        const float e = ccnt >= 0 ? bvh_enter(lo, hi, o, inv, lim0) : __builtin_inff();
        bool oc = false;
        {
            // the overlapped leaf children's triangles, dealt round robin over the quad's lanes
            const uint32_t mine = (ccnt > 0 && e != __builtin_inff()) ? (uint32_t)ccnt : 0u;
            const uint32_t n0 = dpp32<0x00>(mine), n1 = dpp32<0x55>(mine), n2 = dpp32<0xAA>(mine), n3 = dpp32<0xFF>(mine);
            const uint32_t f0 = dpp32<0x00>((uint32_t)cidx), f1 = dpp32<0x55>((uint32_t)cidx);
            const uint32_t f2 = dpp32<0xAA>((uint32_t)cidx), f3 = dpp32<0xFF>((uint32_t)cidx);
            const uint32_t p1 = n0, p2 = n0 + n1, p3 = p2 + n2, tot = p3 + n3;
            constexpr int B = XRT_DEEP_LEAF_BATCH;
            for (uint32_t j0 = (uint32_t)c; j0 < tot; j0 += 4u * B) {
                f4 T[B][3];
                bool ok[B];
#pragma unroll
                for (int b = 0; b < B; ++b) {   // out-of-range slots load triangle 0, unused
                    const uint32_t j = j0 + 4u * (uint32_t)b;
                    ok[b] = j < tot;
                    const uint32_t t = !ok[b] ? 0u : j < p1 ? f0 + j : j < p2 ? f1 + (j - p1) : j < p3 ? f2 + (j - p2)
                                                                                                          : f3 + (j - p3);
                    const size_t i = 3 * (size_t)t;
                    T[b][0] = ldg4(P.bvh_tri, i), T[b][1] = ldg4(P.bvh_tri, i + 1), T[b][2] = ldg4(P.bvh_tri, i + 2);
                }
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    float t;
                    const bool hit = ok[b] && ray_tri_nb(o, d, xyz(T[b][0]), xyz(T[b][1]), xyz(T[b][2]), t);
                    // any hit: area-light objects never occlude (e1.w = occluder flag)
                    oc |= hit && T[b][1].w != 0.0f && t < tmax;
                    const int k = __float_as_int(T[b][2].w);
                    const bool upd = !any && hit && (t < bt || (t == bt && k < bk));
                    bt = upd ? t : bt;
                    bk = upd ? k : bk;
                }
            }
        }
        bool done = any && group_or32<4>(oc ? 1u : 0u) != 0u;
        if (done && c == 0) atomicOr(&occ[id & 63u], 1u << ((id >> 6) - 1u));
        const float lim = any ? tmax : __uint_as_float(group_min32<4>(__float_as_uint(__builtin_fminf(lim0, bt))));
        {
            const bool inner = !done && ccnt == 0 && e <= lim;   // interior child still overlapping [0, lim]
            const uint32_t nkey = inner ? ((__float_as_uint(e) & ~3u) | (uint32_t)c) : ~0u;
            const uint32_t nmin = group_min32<4>(nkey);
            const bool has = nmin != ~0u;
            const bool nearest = inner && nkey == nmin;
            const uint32_t m4 = (uint32_t)(__ballot(inner && !nearest) >> (lane & ~3)) & 0xfu;
            if (inner && !nearest) qs[((sp + __popc(m4 & ((1u << c) - 1u))) & kQsMask) * 16] = (SE)cidx;
            sp += __popc(m4);
            const int child = (int)group_or32<4>(nearest ? (uint32_t)cidx : 0u);
            const bool pop = !done && !has && sp > base;
            const int top_entry = (int)qs[((sp - 1) & kQsMask) * 16];   // read every step; used on a pop
            sp -= pop ? 1 : 0;
            node = has ? child : top_entry;
            done = done || (!has && !pop);
        }
        if (done) {
            if (!any) {   // the quad's closest hit: the smallest (t bits, index) of the lanes
                const uint64_t key = bk >= 0 ? ((uint64_t)__float_as_uint(bt) << 32) | (uint32_t)bk : ~0ull;
                const uint64_t kmin = group_min64<4>(key);
                if (c == 0 && kmin != ~0ull) best[id] = kmin;
            }
            active = false;
        }
    }
}

// After merged_trace<NL, true> over the small objects: rank the rays whose segment still
// reaches the BVH root (the same root test as phase A's queueing, k_trace_2a_coop) into the
// wave's scratch, walk them, and return the merged records.  Must be called by every lane.
template <int NL, typename SE>
__device__ __forceinline__ void deep_pass(const KParams& P, const f4* top, int ntop, SE* stk, MergedWave<NL>& W,
                                          int lane, const f4 (&root)[4], bool ext, v3 o, v3 d, uint32_t shm,
                                          const v3 (&so)[NL + 1], const v3 (&sd)[NL + 1], const float (&stm)[NL + 1],
                                          unsigned long long& best, uint32_t& occ) {
    constexpr int R = 1 + NL;
    bool need[R];
    const float bt = best == ~0ull ? kINF : __uint_as_float((uint32_t)(best >> 32));
    need[0] = ext && root_overlap(root[0], root[1], root[2], root[3], o, rcp3(d), bt);
#pragma unroll
    for (int l = 0; l < NL; ++l)
        need[1 + l] = ((shm & ~occ) >> l & 1u) && root_overlap(root[0], root[1], root[2], root[3], so[l], rcp3(sd[l]), stm[l]);
    wave_sync();   // the last pair pass's reads of W.ro / W.rd are done
    uint32_t tot = 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const uint64_t m = __ballot(need[q]);
        if (need[q]) {
            const uint32_t at = tot + lanemask_rank(m);
            const v3 ro = q == 0 ? o : so[q - 1], rd = q == 0 ? d : sd[q - 1];
            W.ro[at] = make_float4(ro.x, ro.y, ro.z, q == 0 ? kINF : stm[q - 1]);
            W.rd[at] = make_float4(rd.x, rd.y, rd.z, __uint_as_float((uint32_t)(q * 64 + lane)));
        }
        tot += (uint32_t)__popcll(m);
    }
    if (tot == 0) return;
    wave_sync();
    wave_deep_walk<SE>(P, top, ntop, stk, W.ro, W.rd, W.best, W.occ, lane, tot);
    wave_sync();
    best = W.best[lane];
    occ = W.occ[lane];
}

// LDS of k_step_merged<..., BVH = true> (bytes; the f4 regions 16-aligned): the small
// objects' triangles (KParams::stri), the object and light tables, the first ntop 4-wide
// BVH nodes, one MergedWave of trace scratch per wave, then 16 quad stacks of bvh4_stack 16-bit entries per wave
// (use_step_bvh: at most 65,536 nodes).
constexpr uint32_t kStackWave = 16u * kQs * 2u;   // a wave's 16 quad stacks (16-bit entries)
struct BvhStepLayout {
    uint32_t tri, obj, light, top, wave, stack, total;
    int ntop;
};
__host__ __device__ inline BvhStepLayout bvh_step_layout(const KParams& P, uint32_t wave_bytes) {
    BvhStepLayout B;
    B.tri = 0;
    B.obj = 48u * (uint32_t)P.n_stri;
    B.light = B.obj + (uint32_t)sizeof(DObj) * (uint32_t)P.n_objs;
    B.top = (B.light + (uint32_t)sizeof(DLight) * (uint32_t)P.n_lights + 15u) & ~15u;
    // as many of the top XRT_BVH_TOP nodes as the rest leaves room for within kStepLds
    const uint32_t rest = B.top + (kBlock / 64) * wave_bytes + (kBlock / 64) * kStackWave;
    const int fit = rest < kStepLds ? (int)((kStepLds - rest) / 128u) : 0;
    B.ntop = P.bvh4_nodes < XRT_BVH_TOP ? P.bvh4_nodes : XRT_BVH_TOP;
    B.ntop = B.ntop < fit ? B.ntop : fit;
    B.wave = B.top + 128u * (uint32_t)B.ntop;
    B.stack = B.wave + (kBlock / 64) * wave_bytes;
    B.total = B.stack + (kBlock / 64) * kStackWave;
    return B;
}

}  // namespace xrt
