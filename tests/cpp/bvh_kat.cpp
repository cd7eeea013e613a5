// tests/cpp/bvh_kat.cpp — checks the host's hierarchy build (xraytracer_amd/csrc/bvh.h, host/bvh.cpp:
// build_bvh and its breadth-first renumbering, build_bvh_fit, thread_bvh, collapse_bvh4) on its own.
// tests/test_bvh_build.py compiles the two files together, plainly and with
// -fsanitize=address,undefined,float-cast-overflow, and runs the program once per build.
//
// Inputs: every box file named on the command line (written by tests/irregular_meshes.py:
// int32 {n, leaf_max, two_level}, float margin, n x 3 float box minima, n x 3 float box maxima), and
// layouts made here: n = 0 .. leaf_max + 1 boxes, 1,000 identical boxes, 300 boxes whose extents lie
// next to +-FLT_MAX, 3,000 pseudo-random boxes.  For every input, of the first build
// build_bvh(..., KAT_MAX_DEPTH) and of the tree build_bvh_fit returns:
//   * order is a permutation of 0 .. n - 1; the leaves of the binary tree, depth first, left before
//     right, tile [0, n) exactly once; every leaf holds 1 .. leaf_max primitives (0 only for n = 0).
//   * every child box equals the union of its primitives' boxes minus / plus the margin, in float, bit
//     for bit; every child box contains the boxes of the children below it.
//   * every interior index is in range and referenced exactly once; nodes 0 .. min(nn, kBvhTopNodes) - 1
//     are the first nodes of the breadth-first order (left before right); BvhBuild::depth is the
//     deepest child slot found by walking (the root's own slots are at depth 1).
//   * thread_bvh: one node per non-empty child, in depth-first order, with that child's box; skip
//     of node i is the end of i's subtree; "overlap -> i + 1, miss -> skip" from 0 with a ray that
//     overlaps every box visits every leaf once in the binary tree's depth-first order, and with one
//     that misses every box visits the root's children only; the leaf word (count << 24) | first
//     gives count and first back.
//   * collapse_bvh4: the leaves below its root are the binary tree's, each once; every interior child
//     is referenced once and the nodes are in breadth-first order; every child box is the box the
//     binary tree has for the same primitive range; an absent child is (FLT_MAX, -FLT_MAX, count -1);
//     the depth returned is the deepest node found by walking.
//   * stack occupancy, restated from the kernels and simulated for a ray that overlaps every box, in
//     both child orders.  Binary walk (bvh_walk.h bvh_trace, whit_trace.h): leaf children are tested
//     at their parent; of two interior children one is next and the other is pushed, a lone interior
//     child is next without a push, else the walk pops; entries never exceed depth + 1 (bvh_stack).
//     4-wide walk (trace.hip k_trace_deep4 / k_trace_deep4q, wave_deep.h): of a node's interior
//     children one is next and the others (at most three) are pushed, else the walk pops; entries
//     never exceed 3 * depth4 + 1 (bvh4_stack).
//   * fit: build_bvh_fit's tree has depth < KAT_STACK, and for a two-level input 3 * depth4 + 1 <=
//     KAT_STACK4; when the first build fits, it is the tree returned, node for node.
// Per input one line: name, n, nodes, depth, binary stack peak, 4-wide nodes, depth4, 4-wide stack
// peak, threaded nodes, the SAH levels of the tree returned, and FNV-1a hashes of nodes and order:
// `first` of build_bvh's first build with its depth and depth4, `fnv` of the tree returned.  Then
// "ok" and status 0, or the first failure and 1.  With -DKAT_NO_FIT the program needs build_bvh,
// thread_bvh and collapse_bvh4 only and checks and prints the first build alone.
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "bvh.h"

using namespace xrt;

#ifndef KAT_MAX_DEPTH
#define KAT_MAX_DEPTH 48   // wavefront.h kBvhMaxDepth
#endif
#ifndef KAT_STACK
#define KAT_STACK 24       // wavefront.h kBvhStack
#endif
#ifndef KAT_STACK4
#define KAT_STACK4 48      // wavefront.h kBvh4Stack
#endif

struct Input {
    std::string name;
    uint32_t n = 0, leaf_max = 4;
    int two_level = 0;
    float margin = 0.0f;
    std::vector<float> mn, mx;
};

static std::string g_name;
static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
    std::printf("FAIL %s: %s (%ld, %ld, %ld)\n", g_name.c_str(), what, a, b, c);
    return 1;
}

struct B3 {
    float mn[3], mx[3];
};
static bool same(const float* a, const float* b) { return std::memcmp(a, b, 12) == 0; }
static bool inside(const float* imn, const float* imx, const float* omn, const float* omx) {
    for (int q = 0; q < 3; ++q)
        if (!(imn[q] >= omn[q] && imx[q] <= omx[q])) return false;
    return true;
}

static uint64_t fnv1a(const void* p, size_t n, uint64_t h) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
static uint64_t fingerprint(const BvhBuild& b) {
    uint64_t h = 14695981039346656037ull;
    h = fnv1a(b.nodes.data(), b.nodes.size() * sizeof(BvhNode), h);
    return fnv1a(b.order.data(), b.order.size() * sizeof(uint32_t), h);
}

struct Leaf {
    int32_t first, count;
    bool operator==(const Leaf& o) const { return first == o.first && count == o.count; }
};
struct ChildRef {
    const float *mn, *mx;
    int32_t index, count;
};
static ChildRef child_of(const BvhNode& n, int c) {
    return c ? ChildRef{n.rmin, n.rmax, n.right, n.rcount} : ChildRef{n.lmin, n.lmax, n.left, n.lcount};
}

// what a walk of the binary tree finds
struct Walked {
    std::vector<Leaf> leaves;                              // depth first
    std::map<std::pair<uint32_t, uint32_t>, B3> boxes;     // child box by primitive range
    std::vector<int> refs;                                 // references per node
    int depth = 0;
    uint32_t next = 0;                                     // primitives tiled so far
};

// checks the child and returns its primitive range's end; -1 on a failure
static long walk_child(const Input& in, const BvhBuild& b, const ChildRef& ch, int depth, Walked& w) {
    w.depth = std::max(w.depth, depth);
    const uint32_t lo = w.next;
    if (ch.count < 0) return fail("empty child below the root", depth), -1;
    if (ch.count > 0) {
        if ((uint32_t)ch.count > in.leaf_max) return fail("leaf larger than leaf_max", ch.count), -1;
        if ((uint32_t)ch.index != w.next) return fail("leaves do not tile the order", ch.index, w.next), -1;
        w.leaves.push_back(Leaf{ch.index, ch.count});
        w.next += (uint32_t)ch.count;
        if (w.next > in.n) return fail("leaf past the end", ch.index, ch.count), -1;
    } else {
        if (ch.index <= 0 || (size_t)ch.index >= b.nodes.size()) return fail("interior index out of range", ch.index), -1;
        if (++w.refs[(size_t)ch.index] > 1) return fail("node referenced twice", ch.index), -1;
        const BvhNode& nd = b.nodes[(size_t)ch.index];
        for (int c = 0; c < 2; ++c) {
            const ChildRef g = child_of(nd, c);
            if (walk_child(in, b, g, depth + 1, w) < 0) return -1;
            if (!inside(g.mn, g.mx, ch.mn, ch.mx)) return fail("child box outside its parent's", ch.index, c), -1;
        }
    }
    // the box: the union of the primitives' boxes, padded in float
    float umn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, umx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (uint32_t i = lo; i < w.next; ++i) {
        const uint32_t p = b.order[i];
        for (int q = 0; q < 3; ++q) umn[q] = std::min(umn[q], in.mn[3 * p + q]), umx[q] = std::max(umx[q], in.mx[3 * p + q]);
    }
    B3 box;
    for (int q = 0; q < 3; ++q) {
        volatile float a = umn[q] - in.margin, c = umx[q] + in.margin;   // one float rounding each
        box.mn[q] = a, box.mx[q] = c;
    }
    if (!same(box.mn, ch.mn) || !same(box.mx, ch.mx)) return fail("child box is not its primitives' padded union", lo, w.next), -1;
    w.boxes[{lo, w.next}] = box;
    return (long)w.next;
}

// the binary walk's stack for a ray that overlaps every box; order 0: the left child first
static int binary_peak(const BvhBuild& b, int order, std::vector<Leaf>& seen) {
    std::vector<int32_t> stk;
    int peak = 0;
    int32_t node = 0;
    while (true) {
        const BvhNode& n = b.nodes[(size_t)node];
        if (n.lcount > 0) seen.push_back(Leaf{n.left, n.lcount});
        if (n.rcount > 0) seen.push_back(Leaf{n.right, n.rcount});
        const bool il = n.lcount == 0, ir = n.rcount == 0;
        int32_t next = -1;
        if (il && ir) {
            next = order ? n.right : n.left;
            stk.push_back(order ? n.left : n.right);
            peak = std::max(peak, (int)stk.size());
        } else if (il) {
            next = n.left;
        } else if (ir) {
            next = n.right;
        }
        if (next >= 0) {
            node = next;
        } else {
            if (stk.empty()) break;
            node = stk.back(), stk.pop_back();
        }
    }
    return peak;
}

struct Child4 {
    float mn[3], mx[3];
    int32_t index, count;
};
static Child4 child4_of(const Bvh4Node& n, int c) {
    Child4 k;
    std::memcpy(k.mn, n.lo[c], 12), std::memcpy(k.mx, n.hi[c], 12);
    std::memcpy(&k.index, &n.lo[c][3], 4), std::memcpy(&k.count, &n.hi[c][3], 4);
    return k;
}

// the 4-wide walk's stack; order 0: the first interior child is next, 1: the last
static int quad_peak(const std::vector<Bvh4Node>& b4, int order, std::vector<Leaf>& seen) {
    std::vector<int32_t> stk;
    int peak = 0;
    int32_t node = 0;
    while (true) {
        const Bvh4Node& n = b4[(size_t)node];
        std::vector<int32_t> inner;
        for (int c = 0; c < 4; ++c) {
            const Child4 k = child4_of(n, c);
            if (k.count > 0) seen.push_back(Leaf{k.index, k.count});
            if (k.count == 0) inner.push_back(k.index);
        }
        if (!inner.empty()) {
            const size_t pick = order ? inner.size() - 1 : 0;
            for (size_t i = 0; i < inner.size(); ++i)
                if (i != pick) stk.push_back(inner[i]);
            peak = std::max(peak, (int)stk.size());
            node = inner[pick];
        } else {
            if (stk.empty()) break;
            node = stk.back(), stk.pop_back();
        }
    }
    return peak;
}

struct Record {
    size_t nodes = 0, nodes4 = 0, nskip = 0;
    int depth = 0, depth4 = 0, peak = 0, peak4 = 0;
    uint64_t fnv = 0;
};

static bool leaf_less(const Leaf& a, const Leaf& b) { return a.first < b.first; }

// every check of one tree; 0 when they hold
static int check_tree(const Input& in, const BvhBuild& b, Record& rec) {
    const uint32_t n = in.n;
    // ---- order
    if (b.order.size() != n) return fail("order size", (long)b.order.size(), n);
    {
        std::vector<char> seen(n, 0);
        for (uint32_t i = 0; i < n; ++i) {
            if (b.order[i] >= n || seen[b.order[i]]) return fail("order is no permutation", i, b.order[i]);
            seen[b.order[i]] = 1;
        }
    }
    // ---- the binary tree
    const size_t nn = b.nodes.size();
    if (nn == 0) return fail("no root");
    Walked w;
    w.refs.assign(nn, 0);
    const BvhNode& root = b.nodes[0];
    if (n <= in.leaf_max) {   // one leaf and an empty right child
        if (nn != 1) return fail("one-leaf tree with more nodes", (long)nn);
        if (root.rcount != -1 || root.right != 0) return fail("right child of a one-leaf root", root.right, root.rcount);
        for (int q = 0; q < 3; ++q)
            if (root.rmin[q] != FLT_MAX || root.rmax[q] != -FLT_MAX) return fail("empty child's box", q);
        if (n == 0) {
            if (root.lcount != -1) return fail("empty tree's left child", root.lcount);
            w.depth = 1;
        } else if (walk_child(in, b, child_of(root, 0), 1, w) < 0) {
            return 1;
        }
    } else {
        for (int c = 0; c < 2; ++c)
            if (walk_child(in, b, child_of(root, c), 1, w) < 0) return 1;
    }
    if (w.next != n) return fail("leaves do not cover the order", w.next, n);
    for (size_t i = 1; i < nn; ++i)
        if (w.refs[i] != 1) return fail("node not referenced", (long)i);
    if (b.depth != w.depth) return fail("BvhBuild::depth is not the walked depth", b.depth, w.depth);
    {   // breadth first: the first min(nn, kBvhTopNodes) nodes
        std::vector<int32_t> bfs{0};
        for (size_t head = 0; head < bfs.size() && bfs.size() < kBvhTopNodes; ++head)
            for (int c = 0; c < 2; ++c) {
                const ChildRef ch = child_of(b.nodes[(size_t)bfs[head]], c);
                if (ch.count == 0 && bfs.size() < kBvhTopNodes) bfs.push_back(ch.index);
            }
        if (bfs.size() != std::min<size_t>(nn, kBvhTopNodes)) return fail("breadth-first count", (long)bfs.size(), (long)nn);
        for (size_t i = 0; i < bfs.size(); ++i)
            if (bfs[i] != (int32_t)i) return fail("top nodes are not numbered breadth first", (long)i, bfs[i]);
    }
    // ---- the binary walk's stack
    for (int order = 0; order < 2; ++order) {
        std::vector<Leaf> seen;
        const int peak = binary_peak(b, order, seen);
        rec.peak = std::max(rec.peak, peak);
        if (peak > b.depth + 1) return fail("binary walk's stack exceeds depth + 1", peak, b.depth, order);
        std::sort(seen.begin(), seen.end(), leaf_less);
        if (!(seen == w.leaves)) return fail("binary walk does not visit every leaf once", (long)seen.size(), (long)w.leaves.size());
    }
    // ---- the threaded form
    const std::vector<SkipNode> T = thread_bvh(b);
    {
        // expected nodes, depth first: (box, leaf word, end of subtree)
        struct Exp {
            const float *mn, *mx;
            int32_t leaf, skip;
        };
        std::vector<Exp> exp;
        struct Emit {
            const BvhBuild& b;
            std::vector<Exp>& exp;
            void operator()(const ChildRef& ch) {
                if (ch.count < 0) return;
                const size_t me = exp.size();
                exp.push_back(Exp{ch.mn, ch.mx, ch.count > 0 ? (int32_t)(((uint32_t)ch.count << 24) | (uint32_t)ch.index) : -1, 0});
                if (ch.count == 0)
                    for (int c = 0; c < 2; ++c) (*this)(child_of(b.nodes[(size_t)ch.index], c));
                exp[me].skip = (int32_t)exp.size();
            }
        } emit{b, exp};
        emit(child_of(root, 0)), emit(child_of(root, 1));
        if (T.size() != exp.size()) return fail("threaded node count", (long)T.size(), (long)exp.size());
        size_t nonempty = 0;
        for (const BvhNode& nd : b.nodes) nonempty += (nd.lcount >= 0) + (nd.rcount >= 0);
        if (T.size() != nonempty) return fail("threaded nodes are not the non-empty children", (long)T.size(), (long)nonempty);
        for (size_t i = 0; i < T.size(); ++i) {
            if (!same(T[i].bmin, exp[i].mn) || !same(T[i].bmax, exp[i].mx)) return fail("threaded box", (long)i);
            if (T[i].leaf != exp[i].leaf) return fail("threaded leaf word", (long)i, T[i].leaf, exp[i].leaf);
            if (T[i].skip != exp[i].skip || T[i].skip <= (int32_t)i || (size_t)T[i].skip > T.size())
                return fail("threaded skip", (long)i, T[i].skip, exp[i].skip);
        }
        std::vector<Leaf> seen;   // a ray that overlaps every box
        size_t steps = 0;
        for (size_t i = 0; i < T.size(); ++i, ++steps)
            if (T[i].leaf != -1) {
                const uint32_t word = (uint32_t)T[i].leaf;
                const Leaf l{(int32_t)(word & 0xffffffu), (int32_t)(word >> 24)};
                if ((((uint32_t)l.count << 24) | (uint32_t)l.first) != word || l.count < 1) return fail("leaf word", (long)i);
                seen.push_back(l);
            }
        if (!(seen == w.leaves)) return fail("threaded walk's leaves are not the tree's in depth-first order", (long)seen.size());
        size_t i = 0, visits = 0;   // a ray that misses every box
        while (i < T.size()) i = (size_t)T[i].skip, ++visits;
        if (i != T.size() || visits != (size_t)((root.lcount >= 0) + (root.rcount >= 0))) return fail("all-miss walk", (long)visits);
        rec.nskip = T.size();
    }
    // ---- the 4-wide form
    int d4 = -1;
    const std::vector<Bvh4Node> b4 = collapse_bvh4(b, d4);
    {
        if (b4.empty()) return fail("no 4-wide root");
        std::vector<int> refs(b4.size(), 0);
        std::vector<Leaf> leaves;
        int walked = 0;
        // returns the range of the child's primitives through lo / hi
        struct Walk4 {
            const std::vector<Bvh4Node>& b4;
            const Walked& w;
            std::vector<int>& refs;
            std::vector<Leaf>& leaves;
            int& walked;
            int32_t expect = 1;   // breadth-first numbering is checked after the walk
            bool node(int32_t idx, int depth, uint32_t& lo, uint32_t& hi) {
                walked = std::max(walked, depth);
                lo = ~0u, hi = 0;
                const Bvh4Node& n = b4[(size_t)idx];
                int present = 0;
                for (int c = 0; c < 4; ++c) {
                    const Child4 k = child4_of(n, c);
                    uint32_t clo = 0, chi = 0;
                    if (k.count < 0) {
                        if (k.count != -1 || k.index != 0) return fail("absent 4-wide child's words", idx, c), false;
                        for (int q = 0; q < 3; ++q)
                            if (k.mn[q] != FLT_MAX || k.mx[q] != -FLT_MAX) return fail("absent 4-wide child's box", idx, c), false;
                        continue;
                    }
                    if (present != c) return fail("4-wide children are not packed to the front", idx, c), false;
                    ++present;
                    if (k.count > 0) {
                        leaves.push_back(Leaf{k.index, k.count});
                        clo = (uint32_t)k.index, chi = clo + (uint32_t)k.count;
                    } else {
                        if (k.index <= 0 || (size_t)k.index >= b4.size()) return fail("4-wide index out of range", idx, k.index), false;
                        if (++refs[(size_t)k.index] > 1) return fail("4-wide node referenced twice", k.index), false;
                        if (!node(k.index, depth + 1, clo, chi)) return false;
                    }
                    const auto it = w.boxes.find({clo, chi});
                    if (it == w.boxes.end()) return fail("4-wide child's range is no binary child's", idx, clo, chi), false;
                    if (!same(it->second.mn, k.mn) || !same(it->second.mx, k.mx)) return fail("4-wide child box", idx, c), false;
                    lo = std::min(lo, clo), hi = std::max(hi, chi);
                }
                return true;
            }
        } walk4{b4, w, refs, leaves, walked};
        uint32_t lo, hi;
        if (n > 0 && !walk4.node(0, 0, lo, hi)) return 1;
        if (n > 0 && (lo != 0 || hi != n)) return fail("4-wide root's range", lo, hi);
        for (size_t i = 1; i < b4.size(); ++i)
            if (refs[i] != 1) return fail("4-wide node not referenced", (long)i);
        std::sort(leaves.begin(), leaves.end(), leaf_less);
        if (!(leaves == w.leaves)) return fail("4-wide leaves are not the binary tree's", (long)leaves.size(), (long)w.leaves.size());
        if (d4 != walked) return fail("4-wide depth is not the walked depth", d4, walked);
        {   // breadth first, all of it
            int32_t next = 1;
            for (size_t i = 0; i < b4.size(); ++i)
                for (int c = 0; c < 4; ++c) {
                    const Child4 k = child4_of(b4[i], c);
                    if (k.count == 0 && k.index != next++) return fail("4-wide nodes are not numbered breadth first", (long)i, c);
                }
        }
        for (int order = 0; order < 2; ++order) {
            std::vector<Leaf> seen;
            const int peak = quad_peak(b4, order, seen);
            rec.peak4 = std::max(rec.peak4, peak);
            if (peak > 3 * d4 + 1) return fail("4-wide walk's stack exceeds 3 * depth + 1", peak, d4, order);
            std::sort(seen.begin(), seen.end(), leaf_less);
            if (!(seen == w.leaves)) return fail("4-wide walk does not visit every leaf once", (long)seen.size());
        }
    }
    rec.nodes = nn, rec.nodes4 = b4.size(), rec.depth = b.depth, rec.depth4 = d4, rec.fnv = fingerprint(b);
    return 0;
}

static int run(const Input& in) {
    g_name = in.name;
    const BvhBuild first = build_bvh(in.mn.data(), in.mx.data(), in.n, in.leaf_max, in.margin, KAT_MAX_DEPTH);
    Record r1;
    if (check_tree(in, first, r1)) return 1;
#ifdef KAT_NO_FIT
    const Record& r = r1;
    const int levels = KAT_MAX_DEPTH - 24;
#else
    const BvhFit fit = build_bvh_fit(in.mn.data(), in.mx.data(), in.n, in.leaf_max, in.margin, KAT_MAX_DEPTH, KAT_STACK,
                                     in.two_level ? KAT_STACK4 : 0);
    Record r;
    g_name = in.name + " (fit)";
    if (check_tree(in, fit.bvh, r)) return 1;
    const int levels = fit.sah_levels;
    const bool fits = r.depth < KAT_STACK && (!in.two_level || 3 * r.depth4 + 1 <= KAT_STACK4);
    if (!fits || !fit.fits) return fail("the tree returned does not fit the stacks", r.depth, r.depth4, fit.fits);
    if (in.two_level) {
        if (fit.depth4 != r.depth4 || fit.bvh4.size() != r.nodes4) return fail("BvhFit's 4-wide form", fit.depth4, r.depth4);
        int d4 = 0;
        const std::vector<Bvh4Node> again = collapse_bvh4(fit.bvh, d4);
        if (again.size() != fit.bvh4.size() || std::memcmp(again.data(), fit.bvh4.data(), again.size() * sizeof(Bvh4Node)))
            return fail("BvhFit's 4-wide form is not the tree's");
    }
    const bool first_fits = r1.depth < KAT_STACK && (!in.two_level || 3 * r1.depth4 + 1 <= KAT_STACK4);
    if (first_fits && (r.fnv != r1.fnv || levels != KAT_MAX_DEPTH - kBvhMedianLevels))
        return fail("a first build that fits was not kept", levels);
    if (!first_fits && levels >= KAT_MAX_DEPTH - kBvhMedianLevels) return fail("no rebuild of a tree that does not fit", levels);
#endif
    std::printf("%s n=%u two_level=%d nodes=%zu depth=%d peak=%d nodes4=%zu depth4=%d peak4=%d skip=%zu sah_levels=%d "
                "first=%016llx first_depth=%d first_depth4=%d fnv=%016llx\n",
                in.name.c_str(), in.n, in.two_level, r.nodes, r.depth, r.peak, r.nodes4, r.depth4, r.peak4, r.nskip, levels,
                (unsigned long long)r1.fnv, r1.depth, r1.depth4, (unsigned long long)r.fnv);
    return 0;
}

static bool read_input(const char* path, Input& in) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t head[3];
    bool ok = std::fread(head, 4, 3, f) == 3 && std::fread(&in.margin, 4, 1, f) == 1 && head[0] >= 0 && head[1] >= 1;
    if (ok) {
        in.n = (uint32_t)head[0], in.leaf_max = (uint32_t)head[1], in.two_level = head[2];
        in.mn.resize(3 * (size_t)in.n), in.mx.resize(3 * (size_t)in.n);
        ok = std::fread(in.mn.data(), 4, in.mn.size(), f) == in.mn.size() && std::fread(in.mx.data(), 4, in.mx.size(), f) == in.mx.size();
    }
    std::fclose(f);
    const char* slash = std::strrchr(path, '/');
    in.name = slash ? slash + 1 : path;
    return ok;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

static void add_box(Input& in, float x, float y, float z, float sx, float sy, float sz) {
    const float c[3] = {x, y, z}, s[3] = {sx, sy, sz};
    for (int q = 0; q < 3; ++q) in.mn.push_back(c[q]), in.mx.push_back(c[q] + s[q]);
    ++in.n;
}

int main(int argc, char** argv) {
    std::vector<Input> inputs;
    for (uint32_t n = 0; n <= 5; ++n)   // 0 .. leaf_max + 1 boxes in a row
        for (int two = 0; two < 2; ++two) {
            Input in;
            in.name = "row_" + std::to_string(n) + (two ? "_two" : ""), in.margin = 1e-4f, in.two_level = two;
            for (uint32_t i = 0; i < n; ++i) add_box(in, (float)i, 0.5f * (float)i, 0.0f, 0.75f, 0.5f, 0.25f);
            inputs.push_back(in);
        }
    {
        Input in;
        in.name = "identical", in.margin = 1e-4f, in.two_level = 1;
        for (int i = 0; i < 1000; ++i) add_box(in, 3.0f, -2.0f, 7.0f, 1.0f, 2.0f, 0.5f);
        inputs.push_back(in);
    }
    {   // extents next to +-FLT_MAX: the centroids' sum overflows for some (infinite centroids, an infinite
        // or NaN centroid extent, a NaN bin position in Builder::split), the boxes' areas for all
        Input in;
        in.name = "flt_max", in.margin = 1.0f, in.two_level = 1;
        uint32_t s = 7;
        for (int i = 0; i < 300; ++i) {
            const float a = FLT_MAX * (0.5f + 0.5f * unit(s)), b = FLT_MAX * (0.5f + 0.5f * unit(s));
            const float lo[3] = {i % 3 == 0 ? -a : 0.25f * a, i % 3 == 1 ? -b : 0.5f * b, -FLT_MAX};
            const float hi[3] = {i % 3 == 2 ? FLT_MAX : a, b, i % 2 ? FLT_MAX : -0.5f * a};
            for (int q = 0; q < 3; ++q) in.mn.push_back(std::min(lo[q], hi[q])), in.mx.push_back(std::max(lo[q], hi[q]));
            ++in.n;
        }
        inputs.push_back(in);
    }
    for (int two = 0; two < 2; ++two) {
        Input in;
        in.name = two ? "random_two" : "random", in.margin = 1e-3f, in.two_level = two;
        uint32_t s = 12345;
        for (int i = 0; i < 3000; ++i) {
            const float x = 100.0f * unit(s), y = 10.0f * unit(s), z = 50.0f * unit(s);
            add_box(in, x, y, z, 2.0f * unit(s), 0.01f * unit(s), unit(s));
        }
        inputs.push_back(in);
    }
    for (int a = 1; a < argc; ++a) {
        Input in;
        if (!read_input(argv[a], in)) return std::printf("FAIL cannot read %s\n", argv[a]), 1;
        inputs.push_back(std::move(in));
    }
    for (const Input& in : inputs)
        if (run(in)) return 1;
    std::printf("ok\n");
    return 0;
}
