// trace.hip — the trace pass of the wavefront schedule: closest hit for the extension rays and
// any hit for the shadow rays of a compacted slot list, written to the slots' hit records.
//   k_trace       : the linear primitive array, staged through LDS in tiles shared by the block
//   k_trace_small : small triangle scenes, the whole scene in LDS, per-object box culling
//   k_trace_bvh   : large triangle scenes through the host-built BVH (bvh.h, bvh_walk.h)
//   k_trace_2a, k_trace_deep4, k_trace_deep4q : the two-level trace (small objects, then the
//                   BVH walk of the queued rays alone)
// The ray queries (xrt_query) run through the same kernels: k_query_in turns the caller's rays
// into slots, launch_trace traces them, k_query_out rebuilds IntersectInfo from the records.
#include "bvh.h"
#include "bvh_walk.h"
#include "launch.h"
#include "path_common.h"

namespace xrt {

// =================================================================== k_trace ====
template <int SCN, int NL>
__global__ __launch_bounds__(kBlock) void k_trace(KParams P, const uint32_t* __restrict__ list,
                                                   const uint32_t* __restrict__ count, uint32_t* zero_count) {
    __shared__ f4 lds_tri[SCN == SCN_SPHERE ? 1 : 3 * kTriTile];
    __shared__ f4 lds_sph[SCN == SCN_TRI ? 1 : kSphTile];
    __shared__ int lds_sobj[SCN == SCN_TRI ? 1 : kSphTile];
    zero_parts(P, zero_count);
    const PartIter it = part_iter(P, count, kBlock);
    const int tid = threadIdx.x;
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const uint32_t i = base + tid;
        const bool valid = i < it.n;
        const uint32_t s = valid ? list[it.p * P.part_cap + i] : 0;
        const uint32_t st = valid ? P.state[s] : 0;
        const bool want = (st & ST_RAY) != 0;
        const uint32_t smask = (st >> ST_SHADOW_SHIFT) & ((1u << NL) - 1u);
        v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
        if (want) {
            o = xyz(P.ray_o[s]);
            d = xyz(P.ray_d[s]);
        }
        v3 so[NL], sd[NL];
        float stmax[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            so[l] = mk(0, 0, 0), sd[l] = mk(0, 0, 0), stmax[l] = 0.0f;
            if (smask & (1u << l)) {
                const f4 a = P.sh_o[(size_t)l * P.n_slots + s];
                so[l] = xyz(a);
                stmax[l] = a.w;
                sd[l] = xyz(P.sh_d[(size_t)l * P.n_slots + s]);
            }
        }
        uint32_t occ = 0;
        float best_t = kINF, bu = 0.0f, bv = 0.0f;
        int best = -1;
        // mixed scenes: which primitive last wrote SurfaceInfo (position/ng/ns) and which
        // triangle last wrote dpdu/dpdv (spheres and boxes leave them untouched)
        int surf = -1, dp = -1;
        float surf_t = 0.0f, surf_u = 0.0f, surf_v = 0.0f, dp_u = 0.0f, dp_v = 0.0f, t1 = kINF;

        for (int sg = 0; sg < P.n_segs; ++sg) {
            const DSeg seg = P.segs[sg];
            if (SCN != SCN_SPHERE && seg.kind == SEG_TRI) {
                for (int tb = seg.first; tb < seg.first + seg.count; tb += kTriTile) {
                    const int nt = min(kTriTile, seg.first + seg.count - tb);
                    __syncthreads();
                    for (int q = tid; q < 3 * nt; q += kBlock) lds_tri[q] = P.tri[3 * (size_t)tb + q];
                    __syncthreads();
                    for (int k = 0; k < nt; ++k) {
                        const f4 A = lds_tri[3 * k], B = lds_tri[3 * k + 1], Cc = lds_tri[3 * k + 2];
                        const v3 v0 = xyz(A), e1 = xyz(B), e2 = xyz(Cc);
                        if (want) {
                            float t, u, v;
                            if (ray_tri(o, d, v0, e1, e2, t, u, v) && t < best_t) {
                                best_t = t, bu = u, bv = v, best = tb + k;
                                if (SCN == SCN_MIXED) surf = best, surf_t = t, surf_u = u, surf_v = v, dp = best, dp_u = u, dp_v = v;
                            }
                        }
                        if (B.w != 0.0f) {  // occluder (object without an area light)
#pragma unroll
                            for (int l = 0; l < NL; ++l) {
                                if ((smask & (1u << l)) && !(occ & (1u << l))) {
                                    float t, u, v;
                                    if (ray_tri(so[l], sd[l], v0, e1, e2, t, u, v) && t < stmax[l]) occ |= 1u << l;
                                }
                            }
                        }
                    }
                }
            } else if (SCN != SCN_TRI && seg.kind == SEG_SPHERE) {
                for (int tb = seg.first; tb < seg.first + seg.count; tb += kSphTile) {
                    const int nt = min(kSphTile, seg.first + seg.count - tb);
                    __syncthreads();
                    for (int q = tid; q < nt; q += kBlock) {
                        lds_sph[q] = P.sph[tb + q];
                        lds_sobj[q] = P.sph_obj[tb + q];
                    }
                    __syncthreads();
                    for (int k = 0; k < nt; ++k) {
                        const f4 S = lds_sph[k];
                        const v3 c = xyz(S);
                        if (want) {
                            float t;
                            if (sphere_hit(o, d, c, S.w, t) && t < best_t) {
                                best_t = t, bu = 0.0f, bv = 0.0f, best = (1 << 28) | (tb + k);
                                if (SCN == SCN_MIXED) surf = best, surf_t = t;
                            }
                        }
                        if (lds_sobj[k] & (1 << 30)) {
#pragma unroll
                            for (int l = 0; l < NL; ++l) {
                                if ((smask & (1u << l)) && !(occ & (1u << l))) {
                                    float t;
                                    if (sphere_hit(so[l], sd[l], c, S.w, t) && t < stmax[l]) occ |= 1u << l;
                                }
                            }
                        }
                    }
                }
            } else if (SCN == SCN_MIXED && seg.kind == SEG_BOX) {
                for (int b = seg.first; b < seg.first + seg.count; ++b) {
                    const v3 pmin = xyz(P.box[2 * b]), pmax = xyz(P.box[2 * b + 1]);
                    if (want) {
                        float t0, tt1;
                        if (box_hit(o, d, pmin, pmax, t0, tt1)) best_t = t0, t1 = tt1, best = (2 << 28) | b;
                    }
                    // BoxMesh::occluded returns true unconditionally (Src/primitive.h:266-268)
                    occ |= smask;
                }
            }
        }
        if (valid) {
            if (want) {
                P.hit[s] = make_float4(best_t, bu, bv, __int_as_float(best));
                if (SCN == SCN_MIXED) {
                    P.hit2[s] = make_float4(t1, __int_as_float(surf), __int_as_float(dp), surf_t);
                    P.hit3[s] = make_float4(surf_u, surf_v, dp_u, dp_v);
                }
            }
            if (smask) P.occ[s] = occ;
        }
    }
}

// ====================================================================== BVH trace ====
// Large triangle scenes (C4): closest hit and any-hit through the host-built BVH (bvh.h).
// Exactness: every node box is padded beyond the float error of a Moller-Trumbore hit, a
// child is entered when its box overlaps [0, best t] (inclusive: a later triangle at the
// same t with a lower index must still be found), and the closest hit is the
// lexicographic minimum of (t, original index) — the reference's in-order strict
// `t < best` scan over all triangles (Src/scene.cpp:190-200, primitive.cpp:83-131).
// Shadow rays test occluder triangles only and stop at the first hit (Scene::occluded).
// One ray per lane; the traversal stack lives in LDS (kBvhStack entries per thread).

// bvh_leaf / bvh_trace: the per-lane walk, bvh_walk.h

template <int NL, typename SE>
__global__ __launch_bounds__(kBlock) void k_trace_bvh(KParams P, const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ count, uint32_t* zero_count) {
    // LDS: the top min(bvh_nodes, kBvhTopNodes) nodes, then P.bvh_stack * kBlock stack
    // entries of SE (sized to the tree)
    extern __shared__ uint32_t bvh_stack_lds[];
    const int tid = threadIdx.x;
    const int ntop = P.bvh_nodes < (int)kBvhTopNodes ? P.bvh_nodes : (int)kBvhTopNodes;
    f4* top = reinterpret_cast<f4*>(bvh_stack_lds);
    for (int q = tid; q < 4 * ntop; q += kBlock) top[q] = P.bvh_node[q];
    SE* stack = reinterpret_cast<SE*>(bvh_stack_lds + 16 * ntop);
    __syncthreads();
    zero_parts(P, zero_count);
    const PartIter it = part_iter(P, count, kBlock);
    SE* stk = stack + tid;
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const uint32_t i = base + tid;
        if (i >= it.n) continue;
        const uint32_t s = list[it.p * P.part_cap + i];
        const uint32_t st = P.state[s];
        const uint32_t smask = (st >> ST_SHADOW_SHIFT) & ((1u << NL) - 1u);
        if (st & ST_RAY) {
            float bt = kINF, bu = 0.0f, bv = 0.0f;
            int bk = -1;
            (void)bvh_trace<false, SE>(P, top, ntop, stk, xyz(P.ray_o[s]), xyz(P.ray_d[s]), kINF, bt, bu, bv, bk);
            P.hit[s] = make_float4(bt, bu, bv, __int_as_float(bk));
        }
        if (smask) {
            uint32_t occ = 0;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                if (!(smask & (1u << l))) continue;
                const f4 a = P.sh_o[(size_t)l * P.n_slots + s];
                float bt = kINF, bu, bv;
                int bk = -1;
                if (bvh_trace<true, SE>(P, top, ntop, stk, xyz(a), xyz(P.sh_d[(size_t)l * P.n_slots + s]), a.w, bt, bu, bv, bk))
                    occ |= 1u << l;
            }
            P.occ[s] = occ;
        }
    }
}

// ============================================================ two-level trace ====
// Large triangle scenes with small objects beside the big meshes (C4: the Cornell walls and
// blocks around a 51,200-triangle sphere): one wave's rays mostly bounce between the small
// objects, but a single lane whose segment passes the big mesh makes the whole wave walk
// its BVH (k_trace_bvh: lane utilisation 0.12).  Phase A (k_trace_2a) scans the small
// objects as k_trace_small does (LDS, in iteration order, strict t < best: the
// lexicographic (t, index) minimum among them), then queues only the rays whose segment
// [0, best t] (any-hit: [0, tmax], if not yet occluded) overlaps the BVH root; phase B
// (k_trace_deep) walks the BVH for the queued rays alone — full waves of deep rays — and
// merges with the same (t, index) order (bvh_leaf).  The result is the one-level trace's.
template <int NL>
__global__ __launch_bounds__(kBlock) void k_trace_2a(KParams P, const uint32_t* __restrict__ list,
                                                     const uint32_t* __restrict__ count, uint32_t* zero_count) {
    extern __shared__ __attribute__((aligned(16))) f4 lds_2a[];
    f4* ltri = lds_2a;
    DObjBox* lbox = reinterpret_cast<DObjBox*>(lds_2a + 3 * P.n_stri);
    DObjPlane* lpl = reinterpret_cast<DObjPlane*>(lbox + P.n_sobj);
    zero_parts(P, zero_count);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int q = tid; q < 3 * P.n_stri; q += kBlock) ltri[q] = P.stri[q];
    for (int q = tid; q < P.n_sobj; q += kBlock) lbox[q] = P.sbox[q], lpl[q] = P.splane[q];
    __syncthreads();
    const f4 r0 = P.bvh_node[0], r1 = P.bvh_node[1], r2 = P.bvh_node[2], r3 = P.bvh_node[3];   // root
    const PartIter it = part_iter(P, count, kBlock);
    uint32_t* dq = P.deep + (size_t)it.p * P.deep_cap;
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const uint32_t i = base + tid;
        const bool valid = i < it.n;
        const uint32_t s = valid ? list[it.p * P.part_cap + i] : 0;
        const uint32_t st = valid ? P.state[s] : 0;
        const bool want = (st & ST_RAY) != 0;
        const uint32_t smask = (st >> ST_SHADOW_SHIFT) & ((1u << NL) - 1u);
        v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
        if (want) {
            o = xyz(P.ray_o[s]);
            d = xyz(P.ray_d[s]);
        }
        v3 so[NL], sd[NL];
        float stmax[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            so[l] = mk(0, 0, 0), sd[l] = mk(0, 0, 0), stmax[l] = 0.0f;
            if (smask & (1u << l)) {
                const f4 a = P.sh_o[(size_t)l * P.n_slots + s];
                so[l] = xyz(a);
                stmax[l] = a.w;
                sd[l] = xyz(P.sh_d[(size_t)l * P.n_slots + s]);
            }
        }
        const v3 inv = rcp3(d);
        uint32_t occ = 0;
        float best_t = kINF, bu = 0.0f, bv = 0.0f;
        int best = -1;
        for (int ob = 0; ob < P.n_sobj; ++ob) {
            const DObjBox B = lbox[ob];
            const DObjPlane pl = lpl[ob];
            const int cnt = B.count_occ & 0x7fffffff;
            const bool occluder = B.count_occ < 0;
            const bool ne = want && !plane_away_w(o, d, pl) && box_overlap(o, inv, B, best_t);
            uint32_t nsm = 0;
            if (occluder) {
#pragma unroll
                for (int l = 0; l < NL; ++l)
                    if ((smask & ~occ & (1u << l)) && !plane_away_w(so[l], sd[l], pl) &&
                        box_overlap(so[l], rcp3(sd[l]), B, stmax[l]))
                        nsm |= 1u << l;
            }
            if (__ballot(ne || nsm) == 0) continue;
            for (int k = B.first; k < B.first + cnt; ++k) {
                const v3 v0 = xyz(ltri[3 * k]), e1 = xyz(ltri[3 * k + 1]);
                const f4 E2 = ltri[3 * k + 2];
                const v3 e2 = xyz(E2);
                if (ne) {
                    float t, u, v;
                    if (ray_tri(o, d, v0, e1, e2, t, u, v) && t < best_t)
                        best_t = t, bu = u, bv = v, best = __float_as_int(E2.w);
                }
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    if (nsm & ~occ & (1u << l)) {
                        float t, u, v;
                        if (ray_tri(so[l], sd[l], v0, e1, e2, t, u, v) && t < stmax[l]) occ |= 1u << l;
                    }
                }
            }
        }
        const bool dext = want && root_overlap(r0, r1, r2, r3, o, inv, best_t);
        uint32_t dsh = 0;
#pragma unroll
        for (int l = 0; l < NL; ++l)
            if ((smask & ~occ & (1u << l)) && root_overlap(r0, r1, r2, r3, so[l], rcp3(sd[l]), stmax[l])) dsh |= 1u << l;
        if (valid) {
            if (want) P.hit[s] = make_float4(best_t, bu, bv, __int_as_float(best));
            if (smask) P.occ[s] = occ;
        }
        wave_append(valid && dext, s * 8u, dq, P.deep_count + it.p, lane);
#pragma unroll
        for (int l = 0; l < NL; ++l)
            wave_append(valid && ((dsh >> l) & 1u), s * 8u + 1u + (uint32_t)l, dq + P.part_cap,
                        P.deep_count + 2 * kMaxParts + it.p, lane);
    }
}

// bvh_leaf for a leaf of at most kBvhLeaf triangles with every triangle's loads issued before
// the first test (one memory round trip per leaf instead of one per triangle); tests and
// updates in the same order as bvh_leaf.
template <bool ANY>
__device__ __forceinline__ bool bvh_leaf_batch(const KParams& P, int first, int count, v3 o, v3 d, float tmax,
                                               float& bt, float& bu, float& bv, int& bk) {
    f4 T[kBvhLeafTri][3];
#pragma unroll
    for (int q = 0; q < (int)kBvhLeafTri; ++q)
        if (q < count) T[q][0] = P.bvh_tri[3 * (first + q)], T[q][1] = P.bvh_tri[3 * (first + q) + 1],
                       T[q][2] = P.bvh_tri[3 * (first + q) + 2];
#pragma unroll
    for (int q = 0; q < (int)kBvhLeafTri; ++q) {
        if (q >= count) break;
        if (ANY && T[q][1].w == 0.0f) continue;   // area-light objects never occlude
        float t, u, v;
        if (!ray_tri(o, d, xyz(T[q][0]), xyz(T[q][1]), xyz(T[q][2]), t, u, v)) continue;
        if (ANY) {
            if (t < tmax) return true;
        } else {
            const int k = __float_as_int(T[q][2].w);
            if (t < bt || (t == bt && k < bk)) bt = t, bu = u, bv = v, bk = k;
        }
    }
    return false;
}

// Phase B: the queued rays walk the BVH's 4-wide form (bvh.h Bvh4Node: a step fetches four
// child boxes, the tree is about half as deep as the binary one), with dynamic ray fetch —
// a lane whose ray is done takes the next queued ray of its partition (one atomic per wave
// per refill, when at least 16 lanes are idle or the wave is empty), so lanes stay busy
// until the queue drains (a static assignment measured lane utilisation 0.095: most queued
// rays cross the mesh's box and leave after a few nodes, a few descend to the surface).
// One loop iteration = one node per active lane: the four children tested against [0, lim]
// (lim = best t, inclusive, for closest hits; tmax for shadow rays), leaf children first
// (bvh_leaf: the (t, index) order; shadow rays stop at the first occluder), then the nearest
// interior child that still overlaps [0, best t] is next and the other overlapping ones are
// stacked.  Exact for the same reason as bvh_trace: every triangle whose padded box overlaps
// [0, best t] is tested, whatever the order.
template <typename SE>
__global__ __launch_bounds__(kBlock, XRT_DEEP_WAVES) void k_trace_deep4(KParams P) {
    extern __shared__ uint32_t bvh_stack_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ntop = P.bvh4_nodes < (int)kBvhTopNodes ? P.bvh4_nodes : (int)kBvhTopNodes;
    f4* top = reinterpret_cast<f4*>(bvh_stack_lds);
    for (int q = tid; q < 8 * ntop; q += kBlock) top[q] = P.bvh4[q];
    SE* stk = reinterpret_cast<SE*>(bvh_stack_lds + 32 * ntop) + tid;
    __syncthreads();
    const uint32_t p = blockIdx.x % P.n_part;
    // extension rays first, then shadow rays (queued apart by phase A), so a wave's lanes
    // mostly run the same kind of walk (closest hit or any hit) at a time
    const uint32_t n_ext = P.deep_count[p];
    const uint32_t cnt = n_ext + P.deep_count[2 * kMaxParts + p];
    uint32_t* next_ctr = P.deep_count + kMaxParts + p;
    const uint32_t* dq = P.deep + (size_t)p * P.deep_cap;
    const uint32_t* dqs = dq + P.part_cap - n_ext;   // dqs[idx] for idx >= n_ext
#ifdef XRT_EXPERIMENTS
    if (blockIdx.x < P.n_part && tid == 0) atomicAdd(P.stats + 38, (unsigned long long)cnt);
    uint32_t nsteps = 0, niter = 0;
#endif
    bool active = false, drained = cnt == 0, any = false;
    uint32_t s = 0, l = 0;
    int node = 0, sp = 0, bk = -1;
    v3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.0f, bt = kINF, bu = 0.0f, bv = 0.0f;
    while (true) {
#ifdef XRT_EXPERIMENTS
        nsteps += active ? 1u : 0u;
        ++niter;
#endif
        const uint64_t idle = __ballot(!active);
        const uint32_t nidle = (uint32_t)__popcll(idle);
        if (!drained && (nidle >= 16u || nidle == 64u)) {
            const int leader = __ffsll((unsigned long long)idle) - 1;
            uint32_t b = 0;
            if (lane == leader) b = atomicAdd(next_ctr, nidle);
            b = (uint32_t)__builtin_amdgcn_readlane((int)b, leader);
            if (b + nidle >= cnt) drained = true;
            if (!active) {
                const uint32_t idx = b + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                if (idx < cnt) {
                    const uint32_t e = idx < n_ext ? dq[idx] : dqs[idx];
                    s = e >> 3;
                    const uint32_t kind = e & 7u;
                    any = kind != 0;
                    if (!any) {
                        o = xyz(P.ray_o[s]), d = xyz(P.ray_d[s]);
                        const f4 h = P.hit[s];
                        bt = h.x, bu = h.y, bv = h.z, bk = __float_as_int(h.w);
                        tmax = kINF;
                    } else {
                        l = kind - 1u;
                        const f4 a = P.sh_o[(size_t)l * P.n_slots + s];
                        o = xyz(a), tmax = a.w;
                        d = xyz(P.sh_d[(size_t)l * P.n_slots + s]);
                        bt = kINF, bk = -1;
                    }
                    inv = rcp3(d);
                    node = 0, sp = 0;
                    active = true;
                }
            }
        }
        if (!__ballot(active)) break;
        if (!active) continue;
        f4 lo[4], hi[4];
        {
            const f4* N = node < ntop ? top + 8 * node : P.bvh4 + 8 * (size_t)node;
#pragma unroll
            for (int c = 0; c < 4; ++c) lo[c] = N[c], hi[c] = N[4 + c];
        }
        float e[4];
        {
            const float lim = any ? tmax : bt;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                e[c] = __float_as_int(hi[c].w) >= 0 ? bvh_enter(lo[c], hi[c], o, inv, lim) : __builtin_inff();
        }
        bool occluded = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // leaves first (either order gives the same result)
            const int k = __float_as_int(hi[c].w);
            if (!occluded && k > 0 && e[c] != __builtin_inff())
                occluded = any ? bvh_leaf_batch<true>(P, __float_as_int(lo[c].w), k, o, d, tmax, bt, bu, bv, bk)
                               : bvh_leaf_batch<false>(P, __float_as_int(lo[c].w), k, o, d, tmax, bt, bu, bv, bk);
        }
        bool done = occluded;
        if (!done) {
            // interior children still overlapping [0, lim] (bt may have shrunk at the leaves:
            // e <= bt is the same test as a fresh one against the smaller limit)
            const float lim = any ? tmax : bt;
            int nx = -1;
            float en = __builtin_inff();
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (__float_as_int(hi[c].w) != 0 || !(e[c] <= lim)) continue;
                const int idx = __float_as_int(lo[c].w);
                if (nx < 0 || e[c] < en) {
                    if (nx >= 0) stk[(sp++) * kBlock] = (SE)nx;
                    nx = idx, en = e[c];
                } else {
                    stk[(sp++) * kBlock] = (SE)idx;
                }
            }
            if (nx >= 0) node = nx;
            else if (sp == 0) done = true;
            else node = (int)stk[(--sp) * kBlock];
        }
        if (done) {
            if (!any) P.hit[s] = make_float4(bt, bu, bv, __int_as_float(bk));
            else if (occluded) atomicOr(P.occ + s, 1u << l);
            active = false;
        }
    }
#ifdef XRT_EXPERIMENTS
    atomicAdd(P.stats + 39, (unsigned long long)nsteps);
    if (lane == 0) atomicAdd(P.stats + 37, (unsigned long long)niter), atomicMax(P.stats + 36, (unsigned long long)niter);
#endif
}

// Phase B with four lanes per ray ("quad"): lane q of a quad owns child q of the current
// node — loads its two float4, tests its box and, for a leaf child, that leaf's triangles.
// Each lane keeps its own best hit over the triangles it tested (bvh_leaf's (t, index) update
// from the ray's phase-A hit), and the quad shares only what steers the walk, by DPP
// quad_perm: the smallest t as the pruning limit (a 32-bit min per step), occlusion as an or,
// and the next node — the nearest overlapping interior child (key: entry distance with its
// two low bits replaced by the child slot; the order only steers the walk) — with the other
// overlapping ones pushed on one stack per quad.  When the walk ends the quad's closest hit
// is the minimum of the lanes' (t bits, index + 1) keys and the lane holding it writes its
// own (t, u, v, index).  A step costs one node fetch and at most one leaf per lane instead
// of four boxes and up to four leaves, so the longest walk of a launch — which bounds the
// launch when few rays are queued (a row shard of a multi-GPU frame) — takes fewer cycles.
// Exact for the same reason as k_trace_deep4: every triangle whose padded box overlaps
// [0, best t] is tested by some lane (each lane's limit is at least the quad's best t).
// Rays are fetched a quad at a time from the same partitioned queues and counters.
template <typename SE>
__global__ __launch_bounds__(kBlock, XRT_DEEP_WAVES) void k_trace_deep4q(KParams P) {
    extern __shared__ uint32_t bvh_stack_lds[];
    constexpr int kQuads = kBlock / 4;
    const int tid = threadIdx.x, lane = tid & 63, q = lane & 3;
    const int ntop = P.bvh4_nodes < (int)kBvhTopNodes ? P.bvh4_nodes : (int)kBvhTopNodes;
    f4* top = reinterpret_cast<f4*>(bvh_stack_lds);
    for (int i = tid; i < 8 * ntop; i += kBlock) top[i] = P.bvh4[i];
    SE* stk = reinterpret_cast<SE*>(bvh_stack_lds + 32 * ntop) + (tid >> 2);   // one stack per quad
    __syncthreads();
    const uint32_t p = blockIdx.x % P.n_part;
    // extension rays first, then shadow rays (queued apart by phase A), so a wave's lanes
    // mostly run the same kind of walk (closest hit or any hit) at a time
    const uint32_t n_ext = P.deep_count[p];
    const uint32_t cnt = n_ext + P.deep_count[2 * kMaxParts + p];
    uint32_t* next_ctr = P.deep_count + kMaxParts + p;
    const uint32_t* dq = P.deep + (size_t)p * P.deep_cap;
    const uint32_t* dqs = dq + P.part_cap - n_ext;   // dqs[idx] for idx >= n_ext
    constexpr uint64_t kLeads = 0x1111111111111111ull;   // lane 0 of every quad
#ifdef XRT_EXPERIMENTS
    if (blockIdx.x < P.n_part && tid == 0) atomicAdd(P.stats + 38, (unsigned long long)cnt);
    uint32_t nsteps = 0, niter = 0;
#endif
    bool active = false, drained = cnt == 0, any = false;
    uint32_t s = 0, l = 0;
    int node = 0, sp = 0, bk = -1;
    v3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.0f, bt = kINF, bu = 0.0f, bv = 0.0f;
    while (true) {
        const uint64_t idle = __ballot(!active) & kLeads;
        const uint32_t nidle = (uint32_t)__popcll(idle);
        if (!drained && (nidle >= 4u || nidle == 16u)) {
            const int leader = __ffsll((unsigned long long)idle) - 1;
            uint32_t b = 0;
            if (lane == leader) b = atomicAdd(next_ctr, nidle);
            b = (uint32_t)__builtin_amdgcn_readlane((int)b, leader);
            if (b + nidle >= cnt) drained = true;
            if (!active) {
                const uint32_t idx = b + (uint32_t)__popcll(idle & ((1ull << (lane & ~3)) - 1ull));
                if (idx < cnt) {
                    const uint32_t e = idx < n_ext ? dq[idx] : dqs[idx];
                    s = e >> 3;
                    const uint32_t kind = e & 7u;
                    any = kind != 0;
                    if (!any) {
                        o = xyz(P.ray_o[s]), d = xyz(P.ray_d[s]);
                        const f4 h = P.hit[s];
                        bt = h.x, bu = h.y, bv = h.z, bk = __float_as_int(h.w);
                        tmax = kINF;
                    } else {
                        l = kind - 1u;
                        const f4 a = P.sh_o[(size_t)l * P.n_slots + s];
                        o = xyz(a), tmax = a.w;
                        d = xyz(P.sh_d[(size_t)l * P.n_slots + s]);
                        bt = kINF, bk = -1;
                    }
                    inv = rcp3(d);
                    node = 0, sp = 0;
                    active = true;
                }
            }
        }
        if (!__ballot(active)) break;
#ifdef XRT_EXPERIMENTS
        ++niter;
        nsteps += (uint32_t)__popcll(__ballot(active) & kLeads);   // quads stepping (wave-uniform)
#endif
        if (!active) continue;
        // ---- one node: child q on lane q; lim = the quad's best t (closest hits) or tmax
        const f4* N = node < ntop ? top + 8 * node : P.bvh4 + 8 * (size_t)node;
        const f4 lo = N[q], hi = N[4 + q];
        const int cidx = __float_as_int(lo.w), ccnt = __float_as_int(hi.w);
        float lim = any ? tmax : __uint_as_float(group_min32<4>(__float_as_uint(bt)));   // t >= 0: bits order
        const float e = ccnt >= 0 ? bvh_enter(lo, hi, o, inv, lim) : __builtin_inff();
        bool done = false;
        if (any) {
            bool occ = false;
            if (ccnt > 0 && e != __builtin_inff()) occ = bvh_leaf_batch<true>(P, cidx, ccnt, o, d, tmax, bt, bu, bv, bk);
            done = group_or32<4>(occ ? 1u : 0u) != 0u;
            if (done && q == 0) atomicOr(P.occ + s, 1u << l);
        } else {
            if (ccnt > 0 && e != __builtin_inff()) {
                (void)bvh_leaf_batch<false>(P, cidx, ccnt, o, d, kINF, bt, bu, bv, bk);
                lim = __builtin_fminf(lim, bt);   // this lane's leaf may have closed in
            }
            lim = __uint_as_float(group_min32<4>(__float_as_uint(lim)));
        }
        if (!done) {
            const bool inner = ccnt == 0 && e <= lim;   // interior child still overlapping [0, lim]
            const uint32_t nkey = inner ? ((__float_as_uint(e) & ~3u) | (uint32_t)q) : ~0u;
            const uint32_t nmin = group_min32<4>(nkey);
            if (nmin != ~0u) {
                const bool nearest = nkey == nmin;
                const uint32_t m4 = (uint32_t)(__ballot(inner && !nearest) >> (lane & ~3)) & 0xfu;
                if (inner && !nearest) stk[(sp + __popc(m4 & ((1u << q) - 1u))) * kQuads] = (SE)cidx;
                sp += __popc(m4);
                node = (int)group_or32<4>(nearest ? (uint32_t)cidx : 0u);
            } else if (sp == 0) {
                done = true;
            } else {
                node = (int)stk[(--sp) * kQuads];
            }
        }
        if (done) {
            if (!any) {   // the quad's closest hit: the smallest (t bits, index + 1) of the lanes
                const uint64_t key = ((uint64_t)__float_as_uint(bt) << 32) | (uint32_t)(bk + 1);
                const uint64_t kmin = group_min64<4>(key);
                const uint32_t wm = (uint32_t)(__ballot(key == kmin) >> (lane & ~3)) & 0xfu;
                if (q == __builtin_ctz(wm)) P.hit[s] = make_float4(bt, bu, bv, __int_as_float(bk));
            }
            active = false;
        }
    }
#ifdef XRT_EXPERIMENTS
    if (lane == 0)
        atomicAdd(P.stats + 39, (unsigned long long)nsteps), atomicAdd(P.stats + 37, (unsigned long long)niter),
            atomicMax(P.stats + 36, (unsigned long long)niter);
#endif
}

// Small triangle scenes (<= kSmallTris triangles, e.g. the Cornell box): every triangle
// and the per-object boxes live in LDS for the whole launch; objects are visited in
// Scene iteration order and a wave skips an object none of its rays can hit (closest-hit
// rays are culled against the current best t, shadow rays against tmax; area-light
// objects are never occluders).  Inside an object the triangle order and the strict
// `t < best` update are the reference's, so results are identical to the linear scan.
template <int NL>
__global__ __launch_bounds__(kBlock) void k_trace_small(KParams P, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ count, uint32_t* zero_count) {
    extern __shared__ __attribute__((aligned(16))) f4 lds_small[];
    f4* ltri = lds_small;
    DObjBox* lbox = reinterpret_cast<DObjBox*>(lds_small + 3 * P.n_tris);
    zero_parts(P, zero_count);
    const int tid = threadIdx.x;
    for (int q = tid; q < 3 * P.n_tris; q += kBlock) ltri[q] = P.tri[q];
    for (int q = tid; q < P.n_objs; q += kBlock) lbox[q] = P.obj_box[q];
    __syncthreads();
    const PartIter it = part_iter(P, count, kBlock);
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const uint32_t i = base + tid;
        const bool valid = i < it.n;
        const uint32_t s = valid ? list[it.p * P.part_cap + i] : 0;
        const uint32_t st = valid ? P.state[s] : 0;
        const bool want = (st & ST_RAY) != 0;
        const uint32_t smask = (st >> ST_SHADOW_SHIFT) & ((1u << NL) - 1u);
        v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
        if (want) {
            o = xyz(P.ray_o[s]);
            d = xyz(P.ray_d[s]);
        }
        v3 so[NL], sd[NL];
        float stmax[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            so[l] = mk(0, 0, 0), sd[l] = mk(0, 0, 0), stmax[l] = 0.0f;
            if (smask & (1u << l)) {
                const f4 a = P.sh_o[(size_t)l * P.n_slots + s];
                so[l] = xyz(a);
                stmax[l] = a.w;
                sd[l] = xyz(P.sh_d[(size_t)l * P.n_slots + s]);
            }
        }
        const v3 inv = rcp3(d);
        uint32_t occ = 0;
        float best_t = kINF, bu = 0.0f, bv = 0.0f;
        int best = -1;
        for (int ob = 0; ob < P.n_objs; ++ob) {
            const DObjBox B = lbox[ob];
            const int cnt = B.count_occ & 0x7fffffff;
            const bool occluder = B.count_occ < 0;
            const bool ne = want && box_overlap(o, inv, B, best_t);
            uint32_t nsm = 0;
            if (occluder) {
#pragma unroll
                for (int l = 0; l < NL; ++l)
                    if ((smask & ~occ & (1u << l)) && box_overlap(so[l], rcp3(sd[l]), B, stmax[l])) nsm |= 1u << l;
            }
            if (__ballot(ne || nsm) == 0) continue;
            for (int k = B.first; k < B.first + cnt; ++k) {
                const v3 v0 = xyz(ltri[3 * k]), e1 = xyz(ltri[3 * k + 1]), e2 = xyz(ltri[3 * k + 2]);
                if (ne) {
                    float t, u, v;
                    if (ray_tri(o, d, v0, e1, e2, t, u, v) && t < best_t) best_t = t, bu = u, bv = v, best = k;
                }
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    if (nsm & ~occ & (1u << l)) {
                        float t, u, v;
                        if (ray_tri(so[l], sd[l], v0, e1, e2, t, u, v) && t < stmax[l]) occ |= 1u << l;
                    }
                }
            }
        }
        if (valid) {
            if (want) P.hit[s] = make_float4(best_t, bu, bv, __int_as_float(best));
            if (smask) P.occ[s] = occ;
        }
    }
}

// Phase B of the two-level trace (P.two_level): the 4-wide BVH walk of the rays phase A
// queued.  Persistent: up to 2048 blocks (8 per CU), each serving partition blockIdx % n_part.
// A no-op for every other trace.
hipError_t launch_trace_deep(const KParams& P, hipStream_t st) {
    if (!(P.bvh_node && P.scene_kind == SCN_TRI && P.two_level)) return hipSuccess;
    if (!P.bvh4 || P.bvh4_stack <= 0 || P.bvh4_stack > kBvh4Stack) return hipErrorInvalidValue;
    const uint32_t db = P.n_part * std::max<uint32_t>(1u, std::min<uint32_t>(2048u / P.n_part,
                                                                            (P.deep_cap + kBlock - 1) / kBlock));
    const bool small4 = P.bvh4_nodes <= 0x10000;
    const size_t ntop4 = std::min<size_t>((size_t)P.bvh4_nodes, kBvhTopNodes);
    const size_t lds4 = ntop4 * 8 * sizeof(f4) + (size_t)P.bvh4_stack * kBlock * (small4 ? sizeof(uint16_t) : sizeof(uint32_t));
    if (P.deep_quad) {   // four lanes per ray: one stack per quad
        const size_t lds4q = ntop4 * 8 * sizeof(f4) +
                             (size_t)P.bvh4_stack * (kBlock / 4) * (small4 ? sizeof(uint16_t) : sizeof(uint32_t));
        if (small4) hipLaunchKernelGGL((k_trace_deep4q<uint16_t>), dim3(db), dim3(kBlock), lds4q, st, P);
        else hipLaunchKernelGGL((k_trace_deep4q<uint32_t>), dim3(db), dim3(kBlock), lds4q, st, P);
        return hipGetLastError();
    }
    if (small4) hipLaunchKernelGGL((k_trace_deep4<uint16_t>), dim3(db), dim3(kBlock), lds4, st, P);
    else hipLaunchKernelGGL((k_trace_deep4<uint32_t>), dim3(db), dim3(kBlock), lds4, st, P);
    return hipGetLastError();
}

hipError_t launch_trace(const KParams& P, const uint32_t* list, const uint32_t* count, uint32_t* zero,
                        uint32_t blocks, hipStream_t st, bool zero_deep) {
    // every trace kernel has a one-light build and a kMaxLights one
    return with_const<1, kMaxLights>(P.n_lights <= 1 ? 1 : kMaxLights, [&](auto nl) -> hipError_t {
        constexpr int NL = decltype(nl)::value;
        if (P.bvh_node && P.scene_kind == SCN_TRI) {
            if (P.bvh_stack <= 0 || P.bvh_stack > kBvhStack) return hipErrorInvalidValue;
            // node indices below 2^16: 16-bit stack entries, half the LDS per thread
            const bool small = P.bvh_nodes <= 0x10000;
            const size_t ntop = std::min<size_t>((size_t)P.bvh_nodes, kBvhTopNodes);
            const size_t lds =
                ntop * 4 * sizeof(f4) + (size_t)P.bvh_stack * kBlock * (small ? sizeof(uint16_t) : sizeof(uint32_t));
            if (P.two_level) {
                if (!P.deep || !P.deep_count) return hipErrorInvalidValue;
                hipError_t e = zero_deep ? hipMemsetAsync(P.deep_count, 0, 3 * kMaxParts * sizeof(uint32_t), st)   // counts,
                                         : hipSuccess;                                                        // fetch counters
                if (e != hipSuccess) return e;
                const size_t lds_a =
                    (size_t)P.n_stri * 3 * sizeof(f4) + (size_t)P.n_sobj * (sizeof(DObjBox) + sizeof(DObjPlane));
                if (P.sstep)
                    e = launch_trace_2a_coop(P, list, count, zero, blocks, st);
                else
                    hipLaunchKernelGGL((k_trace_2a<NL>), dim3(blocks), dim3(kBlock), lds_a, st, P, list, count, zero);
                if (e == hipSuccess) e = hipGetLastError();
                return e;   // phase B: launch_trace_deep
            }
            if (small)
                hipLaunchKernelGGL((k_trace_bvh<NL, uint16_t>), dim3(blocks), dim3(kBlock), lds, st, P, list, count, zero);
            else
                hipLaunchKernelGGL((k_trace_bvh<NL, uint32_t>), dim3(blocks), dim3(kBlock), lds, st, P, list, count, zero);
            return hipGetLastError();
        }
        if (P.small_tri) {
            const size_t lds = (size_t)P.n_tris * 3 * sizeof(f4) + (size_t)P.n_objs * sizeof(DObjBox);
            hipLaunchKernelGGL((k_trace_small<NL>), dim3(blocks), dim3(kBlock), lds, st, P, list, count, zero);
            return hipGetLastError();
        }
        return with_scene_kind(P.scene_kind, [&](auto scn) {
            hipLaunchKernelGGL((k_trace<decltype(scn)::value, NL>), dim3(blocks), dim3(kBlock), 0, st, P, list, count, zero);
            return hipGetLastError();
        });
    });
}

// ------------------------------------------------------------------ ray queries ----
// Scene::intersect / Scene::occluded for caller rays (xrt_query): the rays become the slots
// of a one-partition list, launch_trace (the render's own trace kernels, BVHs included)
// writes the hit records, and k_query_out rebuilds IntersectInfo with the shading code's
// surface() — the same records the integrators read.
__global__ __launch_bounds__(kBlock) void k_query_in(KParams P, const float* __restrict__ rays,
                                                     const float* __restrict__ tmax, int mode, uint32_t* list,
                                                     uint32_t* count) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s == 0) count[0] = P.n_slots;
    if (s >= P.n_slots) return;
    const float* r = rays + 6 * (size_t)s;
    list[s] = s;
    P.occ[s] = 0;
    if (mode == XRT_QUERY_INTERSECT) {
        P.ray_o[s] = make_float4(r[0], r[1], r[2], 0.0f);
        P.ray_d[s] = make_float4(r[3], r[4], r[5], 0.0f);
        P.state[s] = ST_RAY;
    } else {
        P.sh_o[s] = make_float4(r[0], r[1], r[2], tmax ? tmax[s] : kINF);
        P.sh_d[s] = make_float4(r[3], r[4], r[5], 0.0f);
        P.state[s] = 1u << ST_SHADOW_SHIFT;
    }
}

template <int SCN>
__global__ __launch_bounds__(kBlock) void k_query_out(KParams P, int mode, xrt_hit* __restrict__ out) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P.n_slots) return;
    xrt_hit q;
    memset(&q, 0, sizeof(q));
    q.object = -1, q.primitive = -1;
    if (mode != XRT_QUERY_INTERSECT) {
        q.hit = P.occ[s] & 1u;
        q.t = q.t1 = kINF;
        out[s] = q;
        return;
    }
    const v3 o = xyz(P.ray_o[s]), d = xyz(P.ray_d[s]);
    const f4 h = P.hit[s];
    Surf S;
    float t1;
    const int obj = surface<SCN>(P, s, o, d, h, S, t1);
    // the triangle that last wrote barycentric (with dpdu / dpdv; spheres and boxes leave
    // both untouched), and its (u, v)
    int surf = SCN == SCN_SPHERE ? -1 : __float_as_int(h.w);
    float su = h.y, sv = h.z;
    if (SCN == SCN_MIXED && surf >= 0) {
        const f4 h2 = P.hit2[s], h3 = P.hit3[s];
        surf = __float_as_int(h2.z), su = h3.z, sv = h3.w;
    }
    q.hit = obj >= 0;
    q.object = obj;
    q.primitive = (surf >= 0 && (surf >> 28) == SEG_TRI) ? (surf & 0x0fffffff) : -1;   // global; host makes it local
    q.t = obj >= 0 ? h.x : kINF;
    q.t1 = t1;
    const v3 f[5] = {S.pos, S.ng, S.ns, S.dpdu, S.dpdv};
    float* dst[5] = {q.position, q.ng, q.ns, q.dpdu, q.dpdv};
    for (int k = 0; k < 5; ++k) dst[k][0] = f[k].x, dst[k][1] = f[k].y, dst[k][2] = f[k].z;
    if (q.primitive >= 0) q.barycentric[0] = su, q.barycentric[1] = sv;
    out[s] = q;
}

hipError_t launch_query(const KParams& P, const float* rays, const float* tmax, int mode, uint32_t* list,
                        uint32_t* count, uint32_t* zero, xrt_hit* out, hipStream_t st) {
    const uint32_t blocks = (P.n_slots + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_query_in, dim3(blocks), dim3(kBlock), 0, st, P, rays, tmax, mode, list, count);
    hipError_t e = hipGetLastError();
    // the caller's directions need not be unit vectors, so |det| is not bounded by det_bounded's
    // |e1| |e2|: phase A takes the per-lane test (IEEE-exact reciprocal) instead of the pair passes
    KParams Q = P;
    Q.sstep = nullptr;
    if (e == hipSuccess) e = launch_trace(Q, list, count, zero, blocks, st);
    if (e == hipSuccess) e = launch_trace_deep(Q, st);
    if (e != hipSuccess) return e;
    return with_scene_kind(P.scene_kind, [&](auto scn) {
        hipLaunchKernelGGL(k_query_out<decltype(scn)::value>, dim3(blocks), dim3(kBlock), 0, st, P, mode, out);
        return hipGetLastError();
    });
}

}  // namespace xrt
