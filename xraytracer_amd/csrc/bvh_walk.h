// bvh_walk.h — what the kernels that walk the triangle BVH (bvh.h) share:
//   BvhLds, bvh_lds / bvh4_lds, with_stack_entry, bvh_top_load : the BVH's share of LDS — the top
//       nodes and the traversal stacks — as launchers size it and kernels carve it (trace.hip
//       k_trace_bvh, k_trace_deep4, k_trace_deep4q; whit_trace.h WhitBvhLayout)
//   bvh_leaf, bvh_trace : the per-lane walk (k_trace_bvh; whit_trace.h WhitBvh)
//   plane_away_w        : the small objects' plane cull of the two-level traces
//
// Large triangle scenes (C4): closest hit and any-hit through the host-built BVH (bvh.h).
// Exactness: every node box is padded beyond the float error of a Moller-Trumbore hit, a
// child is entered when its box overlaps [0, best t] (inclusive: a later triangle at the
// same t with a lower index must still be found), and the closest hit is the
// lexicographic minimum of (t, original index) — the reference's in-order strict
// `t < best` scan over all triangles (Src/scene.cpp:190-200, primitive.cpp:83-131).
// Shadow rays test occluder triangles only and stop at the first hit (Scene::occluded).
// One ray per lane; the traversal stack lives in LDS (P.bvh_stack entries per thread,
// STRIDE entries apart: the block's threads interleave their stacks).
#pragma once
#include "bvh.h"
#include "path_common.h"

namespace xrt {

// The BVH's share of a block's LDS: the first ntop nodes (breadth-first: the top of the tree) at
// the start, then from byte `stack` the traversal stacks, whose entries are node indices —
// 16-bit when every index fits (half the LDS per thread), else 32-bit.
struct BvhLds {
    int ntop;               // nodes
    uint32_t node, entry;   // bytes per node; bytes per stack entry
    __host__ __device__ uint32_t stack() const { return (uint32_t)ntop * node; }   // byte offset of the stacks
    // with `stacks` stacks of `depth` entries each
    __host__ __device__ size_t bytes(int depth, int stacks) const { return stack() + (size_t)depth * stacks * entry; }
};
__host__ __device__ inline BvhLds bvh_lds_of(int nodes, uint32_t node_bytes) {
    return {nodes < (int)kBvhTopNodes ? nodes : (int)kBvhTopNodes, node_bytes, nodes <= 0x10000 ? 2u : 4u};
}
__host__ __device__ inline BvhLds bvh_lds(const KParams& P) { return bvh_lds_of(P.bvh_nodes, sizeof(BvhNode)); }
__host__ __device__ inline BvhLds bvh4_lds(const KParams& P) { return bvh_lds_of(P.bvh4_nodes, sizeof(Bvh4Node)); }
// fn(SE{}) with the stack entry type the layout names
template <typename F>
auto with_stack_entry(const BvhLds& B, F&& fn) {
    return B.entry == 2 ? fn(uint16_t{}) : fn(uint32_t{});
}
// the block copies the top nodes to `top`, the start of its dynamic LDS (the caller syncs);
// returns thread 0's stack base
template <typename SE>
__device__ __forceinline__ SE* bvh_top_load(void* top, const f4* nodes, const BvhLds& B, int tid, int stride = kBlock) {
    for (int q = tid; q < B.ntop * (int)(B.node / sizeof(f4)); q += stride) static_cast<f4*>(top)[q] = nodes[q];
    return reinterpret_cast<SE*>(static_cast<char*>(top) + B.stack());
}

template <bool ANY>
__device__ __forceinline__ bool bvh_leaf(const KParams& P, int first, int count, v3 o, v3 d, float tmax, float& bt,
                                         float& bu, float& bv, int& bk) {
    for (int i = first; i < first + count; ++i) {
        const f4 A = P.bvh_tri[3 * i], B = P.bvh_tri[3 * i + 1], C = P.bvh_tri[3 * i + 2];
        if (ANY && B.w == 0.0f) continue;   // area-light objects never occlude
        float t, u, v;
        if (!ray_tri(o, d, xyz(A), xyz(B), xyz(C), t, u, v)) continue;
        if (ANY) {
            if (t < tmax) return true;
        } else {
            const int k = __float_as_int(C.w);
            if (t < bt || (t == bt && k < bk)) bt = t, bu = u, bv = v, bk = k;
        }
    }
    return false;
}

// ANY: returns occluded; else fills (bt, bu, bv, bk) (bk = -1: miss).  Closest-hit rays
// descend into the nearer child first (entry distance) and stack the farther one, so the
// best t shrinks early and culls more of the tree; the result does not depend on the
// order (lexicographic (t, index) minimum over every triangle whose box overlaps).
// top: the first ntop nodes (the breadth-first top of the tree, host/bvh.cpp) in LDS.
// A caller that starts from a hit it already has (bt, bu, bv, bk of the small objects of a
// two-level scene) gets the merge of both: the same (t, index) order decides.
template <bool ANY, typename SE, int STRIDE = kBlock>
__device__ bool bvh_trace(const KParams& P, const f4* top, int ntop, SE* stk, v3 o, v3 d, float tmax, float& bt,
                          float& bu, float& bv, int& bk) {
    const v3 inv = rcp3(d);
    int sp = 0;
    int node = 0;
    while (true) {
        f4 n0, n1, n2, n3;
        if (node < ntop) {
            const f4* N = top + 4 * node;
            n0 = N[0], n1 = N[1], n2 = N[2], n3 = N[3];
        } else {
            const f4* N = P.bvh_node + 4 * (size_t)node;
            n0 = N[0], n1 = N[1], n2 = N[2], n3 = N[3];
        }
        const float lim = ANY ? tmax : bt;
        const int lcount = __float_as_int(n1.w), rcount = __float_as_int(n3.w);
        const float el = lcount >= 0 ? bvh_enter(n0, n1, o, inv, lim) : __builtin_inff();
        const float er = rcount >= 0 ? bvh_enter(n2, n3, o, inv, lim) : __builtin_inff();
        const bool hl = el != __builtin_inff(), hr = er != __builtin_inff();
        // leaves first (either order gives the same result)
        if (hl && lcount > 0 && bvh_leaf<ANY>(P, __float_as_int(n0.w), lcount, o, d, tmax, bt, bu, bv, bk)) return true;
        if (hr && rcount > 0 && bvh_leaf<ANY>(P, __float_as_int(n2.w), rcount, o, d, tmax, bt, bu, bv, bk)) return true;
        const bool il = hl && lcount == 0, ir = hr && rcount == 0;
        int next = -1;
        if (il && ir) {
            const bool lfirst = ANY || el <= er;
            next = __float_as_int(lfirst ? n0.w : n2.w);
            stk[(sp++) * STRIDE] = (SE)__float_as_int(lfirst ? n2.w : n0.w);
        } else if (il) {
            next = __float_as_int(n0.w);
        } else if (ir) {
            next = __float_as_int(n2.w);
        }
        if (next >= 0) {
            node = next;
        } else {
            if (sp == 0) break;
            node = (int)stk[(--sp) * STRIDE];
        }
    }
    return false;
}

// Two-level scenes: the small objects' plane cull (DObjPlane, wavefront.h; merged.h plane_away)
__device__ __forceinline__ bool plane_away_w(v3 o, v3 d, const DObjPlane& pl) {
    const float oa = pl.axis == 0 ? o.x : (pl.axis == 1 ? o.y : o.z);
    const float da = pl.axis == 0 ? d.x : (pl.axis == 1 ? d.y : d.z);
    return pl.axis >= 0 && (oa - pl.c) * da >= 0.0f;
}

}  // namespace xrt
