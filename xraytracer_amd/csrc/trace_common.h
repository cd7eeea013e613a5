// trace_common.h — the steps the trace kernels share (trace.hip, k_trace_2a_coop included):
//   SlotRays / load_slot_rays : a slot's extension ray and shadow rays          (k_trace, k_trace_small,
//                                                                                k_trace_2a, k_trace_2a_coop)
//   SlotHit / write_slot_hit  : the closest hit and occlusion mask of a slot    (k_trace_small, phase A)
//   small_scan                : the LDS scan of small triangle objects          (k_trace_2a; k_trace_small keeps
//                                                                                a written-out copy, for speed)
//   PhaseA / phase_a_finish   : root test, record write, deep-queue appends     (k_trace_2a, k_trace_2a_coop)
//   DeepQueue / deep_fetch    : phase B's queue view and dynamic ray fetch      (k_trace_deep4, k_trace_deep4q)
// The BVH's share of LDS and the per-lane walk are in bvh_walk.h.
#pragma once
#include "bvh_walk.h"
#include "path_common.h"

namespace xrt {

// Entry i of the block's partition: the slot, its extension ray (want) and the shadow rays of
// smask with their tmax.  Lanes past the list's end are invalid and want nothing.  N: the arrays'
// extent (merged_trace takes one element more than NL).
template <int NL, int N = NL>
struct SlotRays {
    bool valid, want;
    uint32_t s, smask;
    v3 o, d;
    v3 so[N], sd[N];
    float stmax[N];
};
template <int NL, int N = NL>
__device__ __forceinline__ SlotRays<NL, N> load_slot_rays(const KParams& P, const uint32_t* __restrict__ list,
                                                          const PartIter& it, uint32_t i) {
    SlotRays<NL, N> R;
    R.valid = i < it.n;
    R.s = R.valid ? list[it.p * P.part_cap + i] : 0;
    const uint32_t st = R.valid ? P.state[R.s] : 0;
    R.want = (st & ST_RAY) != 0;
    R.smask = (st >> ST_SHADOW_SHIFT) & ((1u << NL) - 1u);
    R.o = mk(0, 0, 0), R.d = mk(0, 0, 0);
    if (R.want) {
        R.o = xyz(P.ray_o[R.s]);
        R.d = xyz(P.ray_d[R.s]);
    }
#pragma unroll
    for (int l = 0; l < N; ++l) R.so[l] = mk(0, 0, 0), R.sd[l] = mk(0, 0, 0), R.stmax[l] = 0.0f;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if (R.smask & (1u << l)) {
            const f4 a = P.sh_o[(size_t)l * P.n_slots + R.s];
            R.so[l] = xyz(a);
            R.stmax[l] = a.w;
            R.sd[l] = xyz(P.sh_d[(size_t)l * P.n_slots + R.s]);
        }
    }
    return R;
}

// A slot's trace result: the closest hit (k = -1: miss) and the occluded shadow rays
struct SlotHit {
    float t = kINF, u = 0.0f, v = 0.0f;
    int k = -1;
    uint32_t occ = 0;
};
template <int NL, int N>
__device__ __forceinline__ void write_slot_hit(const KParams& P, const SlotRays<NL, N>& R, const SlotHit& H) {
    if (!R.valid) return;
    if (R.want) P.hit[R.s] = make_float4(H.t, H.u, H.v, __int_as_float(H.k));
    if (R.smask) P.occ[R.s] = H.occ;
}

// The small objects' scan: objects in Scene iteration order from their LDS copy (triangles ltri,
// boxes lbox, PLANES: planes lpl), a wave skipping an object none of its rays can hit (closest-hit
// rays culled against the current best t, shadow rays against tmax; only occluders are tested
// for shadow rays).  Inside an object the triangle order and the strict `t < best` update are
// the reference's, so H is the linear scan's.  ORIG: the reported index is the triangle's
// original one (e2.w, two-level scenes) instead of its position k.  Every lane of the wave calls it.
template <bool PLANES, bool ORIG, int NL>
__device__ __forceinline__ void small_scan(const SlotRays<NL>& R, v3 inv, const f4* ltri, const DObjBox* lbox,
                                           const DObjPlane* lpl, int n_obj, SlotHit& H) {
    for (int ob = 0; ob < n_obj; ++ob) {
        const DObjBox B = lbox[ob];
        DObjPlane pl = {-1, 0.0f};
        if (PLANES) pl = lpl[ob];
        const int cnt = B.count_occ & 0x7fffffff;
        const bool occluder = B.count_occ < 0;
        const bool ne = R.want && !(PLANES && plane_away_w(R.o, R.d, pl)) && box_overlap(R.o, inv, B, H.t);
        uint32_t nsm = 0;
        if (occluder) {
#pragma unroll
            for (int l = 0; l < NL; ++l)
                if ((R.smask & ~H.occ & (1u << l)) && !(PLANES && plane_away_w(R.so[l], R.sd[l], pl)) &&
                    box_overlap(R.so[l], rcp3(R.sd[l]), B, R.stmax[l]))
                    nsm |= 1u << l;
        }
        if (__ballot(ne || nsm) == 0) continue;
        for (int k = B.first; k < B.first + cnt; ++k) {
            const v3 v0 = xyz(ltri[3 * k]), e1 = xyz(ltri[3 * k + 1]);
            const f4 E2 = ltri[3 * k + 2];
            const v3 e2 = xyz(E2);
            if (ne) {
                float t, u, v;
                if (ray_tri(R.o, R.d, v0, e1, e2, t, u, v) && t < H.t)
                    H.t = t, H.u = u, H.v = v, H.k = ORIG ? __float_as_int(E2.w) : k;
            }
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                if (nsm & ~H.occ & (1u << l)) {
                    float t, u, v;
                    if (ray_tri(R.so[l], R.sd[l], v0, e1, e2, t, u, v) && t < R.stmax[l]) H.occ |= 1u << l;
                }
            }
        }
    }
}

// Phase A of the two-level trace ends the same way whatever traced the small objects: a ray
// whose segment [0, best t] (any-hit: [0, tmax], if not yet occluded) overlaps the BVH root is
// queued for phase B — extension rays from the start of the partition's queue, shadow rays
// (entry = slot * 8 + 1 + light) from entry part_cap on — and the slot's record is written.
struct PhaseA {
    f4 r0, r1, r2, r3;   // the BVH root
    uint32_t* dq;        // the partition's queue
    uint32_t *n_ext, *n_sh;
};
__device__ __forceinline__ PhaseA phase_a_begin(const KParams& P, const PartIter& it) {
    return {P.bvh_node[0], P.bvh_node[1], P.bvh_node[2], P.bvh_node[3], P.deep + (size_t)it.p * P.deep_cap,
            P.deep_count + it.p, P.deep_count + 2 * kMaxParts + it.p};
}
// Every lane of the wave calls it (wave_append).
template <int NL, int N>
__device__ __forceinline__ void phase_a_finish(const KParams& P, const PhaseA& A, const SlotRays<NL, N>& R, v3 inv,
                                               const SlotHit& H, int lane) {
    const bool dext = R.want && root_overlap(A.r0, A.r1, A.r2, A.r3, R.o, inv, H.t);
    uint32_t dsh = 0;
#pragma unroll
    for (int l = 0; l < NL; ++l)
        if ((R.smask & ~H.occ & (1u << l)) && root_overlap(A.r0, A.r1, A.r2, A.r3, R.so[l], rcp3(R.sd[l]), R.stmax[l]))
            dsh |= 1u << l;
    write_slot_hit(P, R, H);
    wave_append(R.valid && dext, R.s * 8u, A.dq, A.n_ext, lane);
#pragma unroll
    for (int l = 0; l < NL; ++l)
        wave_append(R.valid && ((dsh >> l) & 1u), R.s * 8u + 1u + (uint32_t)l, A.dq + P.part_cap, A.n_sh, lane);
}

// Phase B's view of partition p's queues: extension rays first, then shadow rays (queued apart
// by phase A), so a wave's lanes mostly run the same kind of walk (closest hit or any hit) at a
// time.  Entry idx is dq[idx] below n_ext and dqs[idx] from there on; next_ctr hands them out.
struct DeepQueue {
    uint32_t n_ext, cnt;
    uint32_t* next_ctr;
    const uint32_t *dq, *dqs;
};
__device__ __forceinline__ DeepQueue deep_queue(const KParams& P, uint32_t p) {
    DeepQueue Q;
    Q.n_ext = P.deep_count[p];
    Q.cnt = Q.n_ext + P.deep_count[2 * kMaxParts + p];
    Q.next_ctr = P.deep_count + kMaxParts + p;
    Q.dq = P.deep + (size_t)p * P.deep_cap;
    Q.dqs = Q.dq + P.part_cap - Q.n_ext;
    return Q;
}
// The ray a lane (LANES_PER_RAY = 1) or a quad (4: every lane holds a copy) is walking
struct DeepRay {
    bool active = false, drained = false, any = false;   // drained: the queue has been handed out
    uint32_t s = 0, l = 0;                               // slot; any: the light
    int node = 0, sp = 0, bk = -1;
    v3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.0f, bt = kINF, bu = 0.0f, bv = 0.0f;
};
// Dynamic ray fetch: idle lanes (quads) take the next queued rays of the partition — one atomic
// per wave per refill, when at least a quarter of the wave's lanes (quads) are idle or all are.
// A closest-hit ray starts from its phase-A hit.  Every lane of the wave calls it.
template <int LANES_PER_RAY>
__device__ __forceinline__ void deep_fetch(const KParams& P, const DeepQueue& Q, DeepRay& R, int lane) {
    constexpr uint32_t kRays = 64 / LANES_PER_RAY;
    constexpr uint64_t kLeads = LANES_PER_RAY == 1 ? ~0ull : 0x1111111111111111ull;   // lane 0 of every quad
    static_assert(LANES_PER_RAY == 1 || LANES_PER_RAY == 4, "a lane or a quad per ray");
    const uint64_t idle = __ballot(!R.active) & kLeads;
    const uint32_t nidle = (uint32_t)__popcll(idle);
    if (R.drained || !(nidle >= kRays / 4 || nidle == kRays)) return;
    const int leader = __ffsll((unsigned long long)idle) - 1;
    uint32_t b = 0;
    if (lane == leader) b = atomicAdd(Q.next_ctr, nidle);
    b = (uint32_t)__builtin_amdgcn_readlane((int)b, leader);
    if (b + nidle >= Q.cnt) R.drained = true;
    if (R.active) return;
    const uint32_t idx = b + (uint32_t)__popcll(idle & ((1ull << (lane & ~(LANES_PER_RAY - 1))) - 1ull));
    if (idx >= Q.cnt) return;
    const uint32_t e = idx < Q.n_ext ? Q.dq[idx] : Q.dqs[idx];
    const uint32_t s = e >> 3, kind = e & 7u;
    // both kinds fill the same locals (stores to different fields on the two sides would be merged
    // into one store through a selected address, which keeps the ray in scratch)
    f4 ro, rd;                                                 // origin and tmax; direction
    f4 h = make_float4(kINF, R.bu, R.bv, __int_as_float(-1));   // a shadow ray starts from a miss
    if (kind == 0) {
        ro = P.ray_o[s], ro.w = kINF;
        rd = P.ray_d[s];
        h = P.hit[s];
    } else {
        R.l = kind - 1u;
        ro = P.sh_o[(size_t)R.l * P.n_slots + s];
        rd = P.sh_d[(size_t)R.l * P.n_slots + s];
    }
    R.s = s, R.any = kind != 0;
    R.o = xyz(ro), R.tmax = ro.w, R.d = xyz(rd), R.inv = rcp3(R.d);
    R.bt = h.x, R.bu = h.y, R.bv = h.z, R.bk = __float_as_int(h.w);
    R.node = 0, R.sp = 0;
    R.active = true;
}

}  // namespace xrt
