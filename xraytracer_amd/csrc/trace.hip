// trace.hip — the trace pass of the wavefront schedule: closest hit for the extension rays and
// any hit for the shadow rays of a compacted slot list, written to the slots' hit records.
//   k_trace       : the linear primitive array, staged through LDS in tiles shared by the block
//   k_trace_small : small triangle scenes, the whole scene in LDS, per-object box culling
//   k_trace_bvh   : large triangle scenes through the host-built BVH (bvh.h, bvh_walk.h)
//   k_trace_2a, k_trace_2a_coop, k_trace_deep4, k_trace_deep4q : the two-level trace (small
//                   objects, then the BVH walk of the queued rays alone)
// What these kernels share is defined once in trace_common.h (the slot ray load, the small-object
// scan, phase A's tail, phase B's queue view and ray fetch) and bvh_walk.h (the BVH's share of LDS,
// the per-lane walk); k_trace_2a_coop's pair passes are the merged step kernels' (merged.h).
// The ray queries (xrt_query) run through the same kernels: k_query_in turns the caller's rays
// into slots, launch_trace traces them, k_query_out rebuilds IntersectInfo from the records.
#include "bvh.h"
#include "bvh_walk.h"
#include "launch.h"
#include "merged.h"
#include "path_common.h"
#include "trace_common.h"

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
        const SlotRays<NL> R = load_slot_rays<NL>(P, list, it, base + tid);
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
                        if (R.want) {
                            float t, u, v;
                            if (ray_tri(R.o, R.d, v0, e1, e2, t, u, v) && t < best_t) {
                                best_t = t, bu = u, bv = v, best = tb + k;
                                if (SCN == SCN_MIXED) surf = best, surf_t = t, surf_u = u, surf_v = v, dp = best, dp_u = u, dp_v = v;
                            }
                        }
                        if (B.w != 0.0f) {  // occluder (object without an area light)
#pragma unroll
                            for (int l = 0; l < NL; ++l) {
                                if ((R.smask & (1u << l)) && !(occ & (1u << l))) {
                                    float t, u, v;
                                    if (ray_tri(R.so[l], R.sd[l], v0, e1, e2, t, u, v) && t < R.stmax[l]) occ |= 1u << l;
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
                        if (R.want) {
                            float t;
                            if (sphere_hit(R.o, R.d, c, S.w, t) && t < best_t) {
                                best_t = t, bu = 0.0f, bv = 0.0f, best = (1 << 28) | (tb + k);
                                if (SCN == SCN_MIXED) surf = best, surf_t = t;
                            }
                        }
                        if (lds_sobj[k] & (1 << 30)) {
#pragma unroll
                            for (int l = 0; l < NL; ++l) {
                                if ((R.smask & (1u << l)) && !(occ & (1u << l))) {
                                    float t;
                                    if (sphere_hit(R.so[l], R.sd[l], c, S.w, t) && t < R.stmax[l]) occ |= 1u << l;
                                }
                            }
                        }
                    }
                }
            } else if (SCN == SCN_MIXED && seg.kind == SEG_BOX) {
                for (int b = seg.first; b < seg.first + seg.count; ++b) {
                    const v3 pmin = xyz(P.box[2 * b]), pmax = xyz(P.box[2 * b + 1]);
                    if (R.want) {
                        float t0, tt1;
                        if (box_hit(R.o, R.d, pmin, pmax, t0, tt1)) best_t = t0, t1 = tt1, best = (2 << 28) | b;
                    }
                    // BoxMesh::occluded returns true unconditionally (Src/primitive.h:266-268)
                    occ |= R.smask;
                }
            }
        }
        if (R.valid) {
            if (R.want) {
                P.hit[R.s] = make_float4(best_t, bu, bv, __int_as_float(best));
                if (SCN == SCN_MIXED) {
                    P.hit2[R.s] = make_float4(t1, __int_as_float(surf), __int_as_float(dp), surf_t);
                    P.hit3[R.s] = make_float4(surf_u, surf_v, dp_u, dp_v);
                }
            }
            if (R.smask) P.occ[R.s] = occ;
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
    // LDS (bvh_lds): the top nodes, then P.bvh_stack * kBlock stack entries of SE
    extern __shared__ uint32_t bvh_stack_lds[];
    const int tid = threadIdx.x;
    const BvhLds B = bvh_lds(P);
    const f4* top = reinterpret_cast<const f4*>(bvh_stack_lds);
    const int ntop = B.ntop;
    SE* stk = bvh_top_load<SE>(bvh_stack_lds, P.bvh_node, B, tid) + tid;
    __syncthreads();
    zero_parts(P, zero_count);
    const PartIter it = part_iter(P, count, kBlock);
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
// objects as k_trace_small does (small_scan: LDS, in iteration order, strict t < best: the
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
    const PartIter it = part_iter(P, count, kBlock);
    const PhaseA A = phase_a_begin(P, it);
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const SlotRays<NL> R = load_slot_rays<NL>(P, list, it, base + tid);
        const v3 inv = rcp3(R.d);
        SlotHit H;
        small_scan<true, true>(R, inv, ltri, lbox, lpl, P.n_sobj, H);
        phase_a_finish(P, A, R, inv, H, lane);
    }
}

// k_trace_2a with the small objects traced by merged_trace's object-major
// pair passes (merged.h) instead of a per-lane object loop: one wave = 64 slots, their extension ray
// and shadow rays, the small objects' triangles in LDS (KParams::stri, iteration order, so
// the (t bits << 32 | local index) minimum is the (t, original index) minimum).  The winner's
// (t, u, v) are recomputed with Mesh::rayTriangleIntersect's ops as the merged kernel does;
// rays whose segment reaches the BVH root are queued for k_trace_deep.
template <int NL>
__global__ __launch_bounds__(kBlock, XRT_2A_WAVES) void k_trace_2a_coop(KParams P, const StepObjs SO, const uint32_t* __restrict__ list,
                                                          const uint32_t* __restrict__ count, uint32_t* zero_count) {
    extern __shared__ __attribute__((aligned(16))) f4 lds_2c[];
    LScene L;
    L.tri = lds_2c;
    MergedWave<NL>* Wv = reinterpret_cast<MergedWave<NL>*>(lds_2c + 3 * P.n_stri);
    const int tid = threadIdx.x, lane = tid & 63;
    MergedWave<NL>& W = Wv[tid >> 6];
    lds_copy(const_cast<f4*>(L.tri), P.stri, 3 * P.n_stri, tid);
    zero_parts(P, zero_count);
    __syncthreads();
    const PartIter it = part_iter(P, count, kBlock);
    const PhaseA A = phase_a_begin(P, it);
    for (uint32_t base = it.first; base < it.n; base += it.stride) {
        const SlotRays<NL, NL + 1> R = load_slot_rays<NL, NL + 1>(P, list, it, base + tid);
        unsigned long long best;
        SlotHit H;
        merged_trace<NL>(SO, L, W, lane, R.want, R.o, R.d, R.smask, R.so, R.sd, R.stmax, best, H.occ);
        if (R.want && best != ~0ull) {
            const int hk = (int)(uint32_t)best;
            (void)ray_tri(R.o, R.d, xyz(L.tri[3 * hk]), xyz(L.tri[3 * hk + 1]), xyz(L.tri[3 * hk + 2]), H.t, H.u, H.v);
            H.k = __float_as_int(L.tri[3 * hk + 2].w);
        }
        H.occ &= R.smask;
        phase_a_finish(P, A, R, rcp3(R.d), H, lane);
        wave_sync();   // W is rewritten by the next round's rays
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
// per refill, when at least 16 lanes are idle or the wave is empty: deep_fetch), so lanes stay busy
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
    const BvhLds B = bvh4_lds(P);
    const f4* top = reinterpret_cast<const f4*>(bvh_stack_lds);
    const int ntop = B.ntop;
    SE* stk = bvh_top_load<SE>(bvh_stack_lds, P.bvh4, B, tid) + tid;
    __syncthreads();
    const DeepQueue Q = deep_queue(P, blockIdx.x % P.n_part);
#ifdef XRT_EXPERIMENTS
    if (blockIdx.x < P.n_part && tid == 0) atomicAdd(P.stats + 38, (unsigned long long)Q.cnt);
    uint32_t nsteps = 0, niter = 0;
#endif
    DeepRay R;
    R.drained = Q.cnt == 0;
    while (true) {
#ifdef XRT_EXPERIMENTS
        nsteps += R.active ? 1u : 0u;
        ++niter;
#endif
        deep_fetch<1>(P, Q, R, lane);
        if (!__ballot(R.active)) break;
        if (!R.active) continue;
        f4 lo[4], hi[4];
        {
            const f4* N = R.node < ntop ? top + 8 * R.node : P.bvh4 + 8 * (size_t)R.node;
#pragma unroll
            for (int c = 0; c < 4; ++c) lo[c] = N[c], hi[c] = N[4 + c];
        }
        float e[4];
        {
            const float lim = R.any ? R.tmax : R.bt;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                e[c] = __float_as_int(hi[c].w) >= 0 ? bvh_enter(lo[c], hi[c], R.o, R.inv, lim) : __builtin_inff();
        }
        bool occluded = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // leaves first (either order gives the same result)
            const int k = __float_as_int(hi[c].w);
            if (!occluded && k > 0 && e[c] != __builtin_inff())
                occluded = R.any ? bvh_leaf_batch<true>(P, __float_as_int(lo[c].w), k, R.o, R.d, R.tmax, R.bt, R.bu, R.bv,
                                                        R.bk)
                                 : bvh_leaf_batch<false>(P, __float_as_int(lo[c].w), k, R.o, R.d, R.tmax, R.bt, R.bu, R.bv,
                                                         R.bk);
        }
        bool done = occluded;
        if (!done) {
            // interior children still overlapping [0, lim] (bt may have shrunk at the leaves:
            // e <= bt is the same test as a fresh one against the smaller limit)
            const float lim = R.any ? R.tmax : R.bt;
            int nx = -1;
            float en = __builtin_inff();
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (__float_as_int(hi[c].w) != 0 || !(e[c] <= lim)) continue;
                const int idx = __float_as_int(lo[c].w);
                if (nx < 0 || e[c] < en) {
                    if (nx >= 0) stk[(R.sp++) * kBlock] = (SE)nx;
                    nx = idx, en = e[c];
                } else {
                    stk[(R.sp++) * kBlock] = (SE)idx;
                }
            }
            if (nx >= 0) R.node = nx;
            else if (R.sp == 0) done = true;
            else R.node = (int)stk[(--R.sp) * kBlock];
        }
        if (done) {
            if (!R.any) P.hit[R.s] = make_float4(R.bt, R.bu, R.bv, __int_as_float(R.bk));
            else if (occluded) atomicOr(P.occ + R.s, 1u << R.l);
            R.active = false;
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
// Rays are fetched a quad at a time from the same partitioned queues and counters (deep_fetch<4>:
// when at least 4 quads are idle or all 16).
template <typename SE>
__global__ __launch_bounds__(kBlock, XRT_DEEP_WAVES) void k_trace_deep4q(KParams P) {
    extern __shared__ uint32_t bvh_stack_lds[];
    constexpr int kQuads = kBlock / 4;
    const int tid = threadIdx.x, lane = tid & 63, q = lane & 3;
    const BvhLds B = bvh4_lds(P);
    const f4* top = reinterpret_cast<const f4*>(bvh_stack_lds);
    const int ntop = B.ntop;
    SE* stk = bvh_top_load<SE>(bvh_stack_lds, P.bvh4, B, tid) + (tid >> 2);   // one stack per quad
    __syncthreads();
    const DeepQueue Q = deep_queue(P, blockIdx.x % P.n_part);
#ifdef XRT_EXPERIMENTS
    constexpr uint64_t kLeads = 0x1111111111111111ull;   // lane 0 of every quad
    if (blockIdx.x < P.n_part && tid == 0) atomicAdd(P.stats + 38, (unsigned long long)Q.cnt);
    uint32_t nsteps = 0, niter = 0;
#endif
    DeepRay R;
    R.drained = Q.cnt == 0;
    while (true) {
        deep_fetch<4>(P, Q, R, lane);
        if (!__ballot(R.active)) break;
#ifdef XRT_EXPERIMENTS
        ++niter;
        nsteps += (uint32_t)__popcll(__ballot(R.active) & kLeads);   // quads stepping (wave-uniform)
#endif
        if (!R.active) continue;
        // ---- one node: child q on lane q; lim = the quad's best t (closest hits) or tmax
        const f4* N = R.node < ntop ? top + 8 * R.node : P.bvh4 + 8 * (size_t)R.node;
        const f4 lo = N[q], hi = N[4 + q];
        const int cidx = __float_as_int(lo.w), ccnt = __float_as_int(hi.w);
        float lim = R.any ? R.tmax : __uint_as_float(group_min32<4>(__float_as_uint(R.bt)));   // t >= 0: bits order
        const float e = ccnt >= 0 ? bvh_enter(lo, hi, R.o, R.inv, lim) : __builtin_inff();
        bool done = false;
        if (R.any) {
            bool occ = false;
            if (ccnt > 0 && e != __builtin_inff())
                occ = bvh_leaf_batch<true>(P, cidx, ccnt, R.o, R.d, R.tmax, R.bt, R.bu, R.bv, R.bk);
            done = group_or32<4>(occ ? 1u : 0u) != 0u;
            if (done && q == 0) atomicOr(P.occ + R.s, 1u << R.l);
        } else {
            if (ccnt > 0 && e != __builtin_inff()) {
                (void)bvh_leaf_batch<false>(P, cidx, ccnt, R.o, R.d, kINF, R.bt, R.bu, R.bv, R.bk);
                lim = __builtin_fminf(lim, R.bt);   // this lane's leaf may have closed in
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
                if (inner && !nearest) stk[(R.sp + __popc(m4 & ((1u << q) - 1u))) * kQuads] = (SE)cidx;
                R.sp += __popc(m4);
                R.node = (int)group_or32<4>(nearest ? (uint32_t)cidx : 0u);
            } else if (R.sp == 0) {
                done = true;
            } else {
                R.node = (int)stk[(--R.sp) * kQuads];
            }
        }
        if (done) {
            if (!R.any) {   // the quad's closest hit: the smallest (t bits, index + 1) of the lanes
                const uint64_t key = ((uint64_t)__float_as_uint(R.bt) << 32) | (uint32_t)(R.bk + 1);
                const uint64_t kmin = group_min64<4>(key);
                const uint32_t wm = (uint32_t)(__ballot(key == kmin) >> (lane & ~3)) & 0xfu;
                if (q == __builtin_ctz(wm)) P.hit[R.s] = make_float4(R.bt, R.bu, R.bv, __int_as_float(R.bk));
            }
            R.active = false;
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
        const SlotRays<NL> R = load_slot_rays<NL>(P, list, it, base + tid);
        const v3 inv = rcp3(R.d);
        SlotHit H;
        // small_scan<false, false> (trace_common.h) written out: through the helper this kernel's
        // launches on the Cornell box at 128 spp took 0.7% longer than the parent's, beyond the
        // parent's own spread in every repetition (profiles/trace_share_ab.json)
        for (int ob = 0; ob < P.n_objs; ++ob) {
            const DObjBox B = lbox[ob];
            const int cnt = B.count_occ & 0x7fffffff;
            const bool occluder = B.count_occ < 0;
            const bool ne = R.want && box_overlap(R.o, inv, B, H.t);
            uint32_t nsm = 0;
            if (occluder) {
#pragma unroll
                for (int l = 0; l < NL; ++l)
                    if ((R.smask & ~H.occ & (1u << l)) && box_overlap(R.so[l], rcp3(R.sd[l]), B, R.stmax[l])) nsm |= 1u << l;
            }
            if (__ballot(ne || nsm) == 0) continue;
            for (int k = B.first; k < B.first + cnt; ++k) {
                const v3 v0 = xyz(ltri[3 * k]), e1 = xyz(ltri[3 * k + 1]), e2 = xyz(ltri[3 * k + 2]);
                if (ne) {
                    float t, u, v;
                    if (ray_tri(R.o, R.d, v0, e1, e2, t, u, v) && t < H.t) H.t = t, H.u = u, H.v = v, H.k = k;
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
        write_slot_hit(P, R, H);
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
    const BvhLds B = bvh4_lds(P);
    return with_stack_entry(B, [&](auto se) {
        using SE = decltype(se);
        if (P.deep_quad)   // four lanes per ray: one stack per quad
            hipLaunchKernelGGL((k_trace_deep4q<SE>), dim3(db), dim3(kBlock), B.bytes(P.bvh4_stack, kBlock / 4), st, P);
        else
            hipLaunchKernelGGL((k_trace_deep4<SE>), dim3(db), dim3(kBlock), B.bytes(P.bvh4_stack, kBlock), st, P);
        return hipGetLastError();
    });
}

hipError_t launch_trace(const KParams& P, const uint32_t* list, const uint32_t* count, uint32_t* zero,
                        uint32_t blocks, hipStream_t st, bool zero_deep) {
    // every trace kernel has a one-light build and a kMaxLights one
    return with_const<1, kMaxLights>(P.n_lights <= 1 ? 1 : kMaxLights, [&](auto nl) -> hipError_t {
        constexpr int NL = decltype(nl)::value;
        if (P.bvh_node && P.scene_kind == SCN_TRI) {
            if (P.bvh_stack <= 0 || P.bvh_stack > kBvhStack) return hipErrorInvalidValue;
            if (P.two_level) {
                if (!P.deep || !P.deep_count) return hipErrorInvalidValue;
                hipError_t e = zero_deep ? hipMemsetAsync(P.deep_count, 0, 3 * kMaxParts * sizeof(uint32_t), st)   // counts,
                                         : hipSuccess;                                                        // fetch counters
                if (e != hipSuccess) return e;
                const size_t lds_a =
                    (size_t)P.n_stri * 3 * sizeof(f4) + (size_t)P.n_sobj * (sizeof(DObjBox) + sizeof(DObjPlane));
                if (P.sstep) {   // the small objects by the merged pair passes
                    const size_t lds_c = (size_t)P.n_stri * 3 * sizeof(f4) + (kBlock / 64) * sizeof(MergedWave<NL>);
                    hipLaunchKernelGGL((k_trace_2a_coop<NL>), dim3(blocks), dim3(kBlock), lds_c, st, P, *P.sstep, list, count, zero);
                } else {
                    hipLaunchKernelGGL((k_trace_2a<NL>), dim3(blocks), dim3(kBlock), lds_a, st, P, list, count, zero);
                }
                if (e == hipSuccess) e = hipGetLastError();
                return e;   // phase B: launch_trace_deep
            }
            const BvhLds B = bvh_lds(P);
            return with_stack_entry(B, [&](auto se) {
                hipLaunchKernelGGL((k_trace_bvh<NL, decltype(se)>), dim3(blocks), dim3(kBlock), B.bytes(P.bvh_stack, kBlock),
                                   st, P, list, count, zero);
                return hipGetLastError();
            });
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
