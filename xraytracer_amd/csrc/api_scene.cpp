// api_scene.cpp — the C ABI of include/xrt.h, what a context renders: the flattened scene with
// its acceleration structures, the camera, the delta lights and the media.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "bvh.h"
#include "ctx.h"
#include "xrt/geometry.h"

using namespace xrt;

static constexpr float kPiF = 3.14159265359;   // Src/geometry.h:10 (float PI), = device_math.h kPI

namespace {

float bits(int x) {
    float f;
    std::memcpy(&f, &x, 4);
    return f;
}

// A triangle of an object lying in the plane x_a = c (e1_a = e2_a = 0 exactly) qualifies for
// the exact plane cull (DObjPlane, plane_away in merged.h) when the
// Moller-Trumbore det and t numerator keep the sign of their exact values: with p, q the
// other two axes, both reduce to (d_a resp. o_a - c) * (e1_p e2_q - e1_q e2_p), each product
// rounded twice and the difference once, so |A - B| must exceed a few ulps of |A| + |B|.
// Nonzero edge components within [1e-6, 1e5] keep every product in the normal range for
// |d_a| >= 1e-20 and |o_a - c| >= 1e-25, and below those |det| resp. |t| stays under
// FLT_EPSILON, so the test rejects without the sign argument.
bool plane_tri_ok(const float* e1, const float* e2, int a) {
    if (e1[a] != 0.0f || e2[a] != 0.0f) return false;
    const int p = (a + 1) % 3, q = (a + 2) % 3;
    for (float x : {e1[p], e1[q], e2[p], e2[q]})
        if (x != 0.0f && !(std::fabs(x) >= 1e-6f && std::fabs(x) <= 1e5f)) return false;
    const double A = (double)e1[p] * e2[q], B = (double)e1[q] * e2[p];
    return std::fabs(A - B) > 1e-4 * (std::fabs(A) + std::fabs(B));
}

// The scene in the device's layout, on the host: what flatten_scene makes of an
// xrt_scene_desc and the acceleration structures are built from.
struct FlatScene {
    std::vector<f4> tri, tri_ng, tri_nrm, sph, box;
    std::vector<int> sph_obj;
    std::vector<DObj> objs;
    std::vector<int> obj_count;      // xrt_object.count
    std::vector<float> raw_albedo;   // xrt_object.albedo, 3 per object (k_aov)
    std::vector<DSeg> segs;
    std::vector<DLight> lights;
    std::vector<DObjPlane> planes;   // per object: the plane a mesh lies in (axis -1: none)
    std::vector<int> tri_first;      // per object: its first triangle (-1: not a mesh)
    double emax = 0.0;               // largest |e1| |e2| of a triangle (bounds |det| of every ray test)
    bool has_mirror = false, has_glass = false;
    bool all_lambert = true;         // every object that is no light is a Lambert (use_step_spec)

    // object k's flags in DObjBox::count_occ
    int count_occ(size_t k) const { return obj_count[k] | (objs[k].light < 0 ? (int)0x80000000 : 0); }
};

// Flattened Scene -> device layout, with every check of the description.  Primitives are
// re-packed in object iteration order, so the linear scan order equals Scene::intersect's
// order (Src/scene.cpp:190-200).
int flatten_scene(xrt_ctx* c, const xrt_scene_desc* s, FlatScene& F) {
    if (s->n_lights > (uint32_t)kMaxLights)
        return set_err(c, XRT_ERR_UNSUPPORTED, "more than " + std::to_string(kMaxLights) + " area lights");
    if ((s->n_objects && !s->objects) || (s->n_lights && !s->lights))
        return set_err(c, XRT_ERR_INVALID, "null scene arrays");
    F.tri_first.assign(s->n_objects, -1);
    F.planes.assign(s->n_objects, DObjPlane{-1, 0.0f});
    auto V = [](const float* p) { return Vec3f(p[0], p[1], p[2]); };
    auto F4 = [](const Vec3f& v, float w) { return f4{v[0], v[1], v[2], w}; };
    for (uint32_t k = 0; k < s->n_objects; ++k) {
        const xrt_object& o = s->objects[k];
        F.has_mirror = F.has_mirror || o.material == XRT_MAT_METAL || o.material == XRT_MAT_GLASS;
        F.has_glass = F.has_glass || o.material == XRT_MAT_GLASS;
        F.all_lambert = F.all_lambert && (o.light >= 0 || o.material == XRT_MAT_LAMBERT);
        if (o.light >= (int)s->n_lights || o.count < 0 || o.first < 0)
            return set_err(c, XRT_ERR_INVALID, "object " + std::to_string(k) + ": bad light index or range");
        DObj d{};
        d.kind = o.kind, d.material = o.material, d.light = o.light, d.medium = o.medium;
        for (int q = 0; q < 3; ++q) d.fr[q] = o.material == 1 ? o.albedo[q] / kPiF : 0.0f;
        F.objs.push_back(d);
        F.obj_count.push_back(o.count);
        F.raw_albedo.insert(F.raw_albedo.end(), o.albedo, o.albedo + 3);
        const bool occluder = o.light < 0;  // Scene::occluded skips area-light objects
        int kind = -1, first = 0;
        uint32_t axes = 0;   // meshes: DObjPlane candidates
        if (o.kind == XRT_OBJ_MESH) {
            if ((uint64_t)o.first + o.count > s->n_tris || (o.count && (!s->tri_v || !s->tri_n)))
                return set_err(c, XRT_ERR_INVALID, "mesh range out of bounds");
            kind = SEG_TRI;
            first = (int)(F.tri.size() / 3);
            F.tri_first[k] = first;
            axes = o.count > 0 ? 7u : 0u;   // axes on which every vertex so far shares v[0]'s coordinate
            const float* vfirst = s->tri_v + 9 * (size_t)o.first;
            for (int t = o.first; t < o.first + o.count; ++t) {
                const float* v = s->tri_v + 9 * (size_t)t;
                const float* n = s->tri_n + 9 * (size_t)t;
                const Vec3f v0 = V(v), v1 = V(v + 3), v2 = V(v + 6);
                const Vec3f e1 = v1 - v0, e2 = v2 - v0;     // Src/primitive.cpp:142-143
                F.emax = std::max(F.emax, std::sqrt((double)dot(e1, e1) * (double)dot(e2, e2)));
                for (int a = 0; a < 3; ++a)
                    if (!(v[a] == vfirst[a] && v[3 + a] == vfirst[a] && v[6 + a] == vfirst[a]) ||
                        !plane_tri_ok(e1.getPtr(), e2.getPtr(), a))
                        axes &= ~(1u << a);
                F.tri.push_back(F4(v0, bits((int)k)));
                F.tri.push_back(F4(e1, occluder ? 1.0f : 0.0f));
                F.tri.push_back(F4(e2, 0.0f));
                F.tri_ng.push_back(F4(normalize(cross(e1, e2)), 0.0f));   // Src/primitive.cpp:106
                F.tri_nrm.push_back(F4(V(n), 0.0f));
                F.tri_nrm.push_back(F4(V(n + 3), 0.0f));
                F.tri_nrm.push_back(F4(V(n + 6), 0.0f));
            }
        } else if (o.kind == XRT_OBJ_SPHERE) {
            if ((uint64_t)o.first + o.count > s->n_spheres || !s->spheres)
                return set_err(c, XRT_ERR_INVALID, "sphere range out of bounds");
            kind = SEG_SPHERE;
            first = (int)F.sph.size();
            for (int t = o.first; t < o.first + o.count; ++t) {
                const float* p = s->spheres + 4 * (size_t)t;
                F.sph.push_back(f4{p[0], p[1], p[2], p[3]});
                F.sph_obj.push_back((int)k | (occluder ? (1 << 30) : 0));
            }
        } else if (o.kind == XRT_OBJ_BOX) {
            if ((uint64_t)o.first + o.count > s->n_boxes || !s->boxes)
                return set_err(c, XRT_ERR_INVALID, "box range out of bounds");
            kind = SEG_BOX;
            first = (int)(F.box.size() / 2);
            for (int t = o.first; t < o.first + o.count; ++t) {
                const float* p = s->boxes + 6 * (size_t)t;
                F.box.push_back(f4{p[0], p[1], p[2], bits((int)k)});
                F.box.push_back(f4{p[3], p[4], p[5], 0.0f});
            }
        } else {
            return set_err(c, XRT_ERR_INVALID, "unknown object kind");
        }
        if (kind == SEG_TRI && o.count > 0) {
            for (int a = 0; a < 3; ++a)
                if ((axes >> a) & 1u) {
                    F.planes[k] = DObjPlane{a, s->tri_v[9 * (size_t)o.first + a]};
                    break;
                }
        }
        if (o.count == 0) continue;
        if (!F.segs.empty() && F.segs.back().kind == kind && F.segs.back().first + F.segs.back().count == first)
            F.segs.back().count += o.count;
        else
            F.segs.push_back(DSeg{kind, first, o.count, 0});
    }
    for (uint32_t l = 0; l < s->n_lights; ++l) {
        const xrt_light& L = s->lights[l];
        if (L.kind < XRT_LIGHT_QUAD || L.kind > XRT_LIGHT_SPHERE_AREA)
            return set_err(c, XRT_ERR_INVALID, "light " + std::to_string(l) + ": unknown kind");
        DLight d{};
        d.kind = L.kind;
        const Vec3f v0 = V(L.v0), v1 = V(L.v1), v2 = V(L.v2);
        const Vec3f e1 = v1 - v0, e2 = v2 - v0, Ng = cross(e1, e2);   // QuadLight/TriangleLight ctor
        for (int q = 0; q < 3; ++q) {
            d.v0[q] = v0[q], d.v1[q] = v1[q], d.v2[q] = v2[q];
            d.e1[q] = e1[q], d.e2[q] = e2[q], d.Ng[q] = Ng[q];
            d.center[q] = L.center[q], d.Le[q] = L.Le[q];
        }
        d.radius = L.radius;
        F.lights.push_back(d);
    }
    return XRT_OK;
}

// the flat arrays onto the device, and the parameters that follow from them alone
int upload_flat(xrt_ctx* c, const FlatScene& F) {
    int rc;
    if ((rc = upload(c, c->tri, F.tri.data(), F.tri.size() * sizeof(f4))) ||
        (rc = upload(c, c->tri_ng, F.tri_ng.data(), F.tri_ng.size() * sizeof(f4))) ||
        (rc = upload(c, c->tri_nrm, F.tri_nrm.data(), F.tri_nrm.size() * sizeof(f4))) ||
        (rc = upload(c, c->sph, F.sph.data(), F.sph.size() * sizeof(f4))) ||
        (rc = upload(c, c->sph_obj, F.sph_obj.data(), F.sph_obj.size() * sizeof(int))) ||
        (rc = upload(c, c->box, F.box.data(), F.box.size() * sizeof(f4))) ||
        (rc = upload(c, c->objs, F.objs.data(), F.objs.size() * sizeof(DObj))) ||
        (rc = upload(c, c->obj_albedo, F.raw_albedo.data(), F.raw_albedo.size() * sizeof(float))) ||
        (rc = upload(c, c->lights, F.lights.data(), F.lights.size() * sizeof(DLight))) ||
        (rc = upload(c, c->segs, F.segs.data(), F.segs.size() * sizeof(DSeg))))
        return rc;
    KParams& P = c->base;
    P.tri = as<f4>(c->tri), P.tri_ng = as<f4>(c->tri_ng), P.tri_nrm = as<f4>(c->tri_nrm);
    P.sph = as<f4>(c->sph), P.sph_obj = as<int>(c->sph_obj), P.box = as<f4>(c->box);
    P.objs = as<DObj>(c->objs), P.lights = as<DLight>(c->lights), P.segs = as<DSeg>(c->segs);
    P.n_segs = (int)F.segs.size(), P.n_lights = (int)F.lights.size();
    P.n_tris = (int)(F.tri.size() / 3), P.n_sph = (int)F.sph.size(), P.n_box = (int)(F.box.size() / 2);
    bool only_tri = true, only_sph = true;
    for (const DSeg& g : F.segs) only_tri &= g.kind == SEG_TRI, only_sph &= g.kind == SEG_SPHERE;
    P.scene_kind = (only_tri || F.segs.empty()) ? SCN_TRI : (only_sph ? SCN_SPHERE : SCN_MIXED);
    P.n_objs = (int)F.objs.size();
    // |det| = |e1 . (d x e2)| <= |e1| |e2| |d| with |d| = 1 (+ a few ulp) for every traced ray,
    // so below 2^120 every finite det is either < kEPSILON (rejected whatever 1/det is) or in
    // rcp_newton's exact range: ray_tri_nb then skips the IEEE fallback (det_bounded).
    P.det_bounded = F.emax < 0x1p120 ? 1 : 0;   // NaN / inf edges: false
    P.all_lambert = F.all_lambert ? 1 : 0;
    return XRT_OK;
}

// The scene's bounds, grown box by box.  The boxes of an acceleration structure are padded
// by pad(k) = k of the scene diagonal + k, far above the float error of a hit position, so a
// box test never drops a hit the linear scan accepts.
struct Bounds {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    void grow(const float* bmn, const float* bmx) {
        for (int q = 0; q < 3; ++q) lo[q] = std::min(lo[q], bmn[q]), hi[q] = std::max(hi[q], bmx[q]);
    }
    float pad(float k) const {
        const float diag = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) +
                                     (hi[2] - lo[2]) * (hi[2] - lo[2]));
        return k * diag + k;
    }
};

// triangle t's box (vertices v0, v0 + e1, v0 + e2 as the device sees them); grows the scene's
void tri_box(const std::vector<f4>& tri, size_t t, float* bmn, float* bmx, Bounds& scene) {
    const f4 v0 = tri[3 * t], e1 = tri[3 * t + 1], e2 = tri[3 * t + 2];
    const float vs[3][3] = {{v0.x, v0.y, v0.z}, {v0.x + e1.x, v0.y + e1.y, v0.z + e1.z},
                            {v0.x + e2.x, v0.y + e2.y, v0.z + e2.z}};
    for (int q = 0; q < 3; ++q) {
        bmn[q] = std::min({vs[0][q], vs[1][q], vs[2][q]});
        bmx[q] = std::max({vs[0][q], vs[1][q], vs[2][q]});
    }
    scene.grow(bmn, bmx);
}

// an object's box, unpadded, over the triangles `index(i)` names for i in [b.first, b.first + count)
template <typename Index>
void object_box(const std::vector<f4>& tri, DObjBox& b, Index&& index, Bounds& scene) {
    for (int q = 0; q < 3; ++q) b.bmin[q] = 3e38f, b.bmax[q] = -3e38f;
    for (int i = b.first; i < b.first + (b.count_occ & 0x7fffffff); ++i) {
        float bmn[3], bmx[3];
        tri_box(tri, index(i), bmn, bmx, scene);
        for (int q = 0; q < 3; ++q) b.bmin[q] = std::min(b.bmin[q], bmn[q]), b.bmax[q] = std::max(b.bmax[q], bmx[q]);
    }
}

void pad_boxes(std::vector<DObjBox>& boxes, float margin) {
    for (DObjBox& b : boxes)
        for (int q = 0; q < 3; ++q) b.bmin[q] -= margin, b.bmax[q] += margin;
}

// small triangle scenes: per-object culling boxes (padded by 1e-3) and planes for
// k_trace_small and the merged-trace schedule
int build_small_scene(xrt_ctx* c, const FlatScene& F) {
    KParams& P = c->base;
    P.small_tri = 0;
    if (!(P.scene_kind == SCN_TRI && P.n_tris <= kSmallTris && P.n_objs <= kSmallObjs && P.n_tris > 0)) return XRT_OK;
    Bounds scene;
    std::vector<DObjBox> boxes(F.objs.size());
    int t0 = 0;
    for (size_t k = 0; k < F.objs.size(); ++k) {
        boxes[k].first = t0;
        boxes[k].count_occ = F.count_occ(k);
        object_box(F.tri, boxes[k], [](int t) { return (size_t)t; }, scene);
        t0 += F.obj_count[k];
    }
    pad_boxes(boxes, scene.pad(1e-3f));
    int rc;
    if ((rc = upload(c, c->obj_box, boxes.data(), boxes.size() * sizeof(DObjBox))) ||
        (rc = upload(c, c->obj_plane, F.planes.data(), F.planes.size() * sizeof(DObjPlane))))
        return rc;
    P.obj_box = as<DObjBox>(c->obj_box);
    P.obj_plane = as<DObjPlane>(c->obj_plane);
    if (boxes.size() <= (size_t)kMergedMaxObjs)
        build_step_objs(boxes.data(), F.planes.data(), (int)boxes.size(), c->step_objs);
    P.small_tri = 1;
    return XRT_OK;
}

// large triangle scenes: a BVH (padded by 1e-4) for the wavefront trace (C4's 51k-triangle
// sphere mesh), and the two-level split of it
int build_tri_bvh(xrt_ctx* c, const FlatScene& F) {
    KParams& P = c->base;
    P.bvh_node = nullptr, P.bvh_tri = nullptr, P.bvh_stack = 0, P.bvh_nodes = 0;
    P.stri = nullptr, P.sbox = nullptr, P.splane = nullptr, P.n_stri = 0, P.n_sobj = 0, P.two_level = 0;
    P.sstep = nullptr, P.bvh4 = nullptr, P.bvh4_nodes = 0, P.bvh4_stack = 0, P.deep_quad = 0;
    c->bvh_tris = 0;
    if (!(P.scene_kind == SCN_TRI && !P.small_tri && P.n_tris > 0 && !exp_env("XRT_NO_BVH"))) return XRT_OK;
    const std::vector<f4>& tri = F.tri;
    // two-level split: mesh objects of more than kLargeObjTris triangles go into the BVH,
    // the rest (if any, and if they fit the LDS scan) are scanned directly
    std::vector<uint32_t> big;   // original indices of the BVH's triangles
    std::vector<DObjBox> sboxes;
    std::vector<DObjPlane> splanes;
    std::vector<f4> stri;
    {
        int t0 = 0;
        for (size_t k = 0; k < F.objs.size(); ++k) {
            const int cnt = F.obj_count[k];
            if (cnt > kLargeObjTris) {
                for (int t = t0; t < t0 + cnt; ++t) big.push_back((uint32_t)t);
            } else if (cnt > 0) {
                DObjBox b;
                b.first = (int)(stri.size() / 3);
                b.count_occ = F.count_occ(k);
                for (int t = t0; t < t0 + cnt; ++t) {
                    stri.push_back(tri[3 * t]), stri.push_back(tri[3 * t + 1]), stri.push_back(tri[3 * t + 2]);
                    stri.back().w = bits(t);
                }
                sboxes.push_back(b);
                splanes.push_back(F.planes[k]);
            }
            t0 += cnt;
        }
    }
    const bool two = !big.empty() && !sboxes.empty() && stri.size() / 3 <= (size_t)kSmallTris &&
                     sboxes.size() <= (size_t)kSmallObjs && !exp_env("XRT_NO_TWO_LEVEL");
    if (!two) {
        big.resize(P.n_tris);
        for (size_t t = 0; t < big.size(); ++t) big[t] = (uint32_t)t;
    }
    // A triangle with an exactly zero edge vector (two equal vertices, e.g. half of a
    // SphereMesh's pole cells) is rejected by every Moller-Trumbore test: e1 = 0 makes
    // det = e1 . pvec an exact 0, e2 = 0 makes pvec = d x e2 an exact 0 (a NaN direction
    // fails t > eps instead) — so it is left out of the BVH, where its box would overlap
    // every other pole triangle's.
    {
        auto zero = [](const f4& e) { return e.x == 0.0f && e.y == 0.0f && e.z == 0.0f; };
        size_t w = 0;
        for (size_t i = 0; i < big.size(); ++i)
            if (!zero(tri[3 * big[i] + 1]) && !zero(tri[3 * big[i] + 2])) big[w++] = big[i];
        if (w > 0) big.resize(w);
    }
    const size_t nt = big.size();
    std::vector<float> mn(3 * nt), mx(3 * nt);
    Bounds scene;
    for (size_t i = 0; i < nt; ++i) tri_box(tri, big[i], &mn[3 * i], &mx[3 * i], scene);
    int rc;
    if (two) {   // the small objects: the small-scene scan's boxes (the scene diagonal covers them too)
        for (DObjBox& b : sboxes)
            object_box(tri, b, [&](int i) { return (size_t)__builtin_bit_cast(int, stri[3 * i + 2].w); }, scene);
        pad_boxes(sboxes, scene.pad(1e-3f));
        if ((rc = upload(c, c->stri, stri.data(), stri.size() * sizeof(f4))) ||
            (rc = upload(c, c->sbox, sboxes.data(), sboxes.size() * sizeof(DObjBox))) ||
            (rc = upload(c, c->splane, splanes.data(), splanes.size() * sizeof(DObjPlane))))
            return rc;
        P.stri = as<f4>(c->stri), P.sbox = as<DObjBox>(c->sbox), P.splane = as<DObjPlane>(c->splane);
        P.n_stri = (int)(stri.size() / 3), P.n_sobj = (int)sboxes.size(), P.two_level = 1;
        if (sboxes.size() <= (size_t)kMergedMaxObjs) {   // phase A as cooperative pair passes
            build_step_objs(sboxes.data(), splanes.data(), (int)sboxes.size(), c->sstep);
            P.sstep = P.det_bounded ? &c->sstep : nullptr;   // k_trace_2a_coop: ray_tri_nb
        }
    }
    // the SAH tree when the walks' stacks hold it (every scene with a reasonably even mesh), else
    // one with fewer SAH levels: a mesh that spans many octaves of scale lets SAH peel a bin off
    // per level, and the reference renders it all the same
    const BvhFit fit = build_bvh_fit(mn.data(), mx.data(), (uint32_t)nt, kBvhLeafTri, scene.pad(1e-4f), kBvhMaxDepth,
                                     kBvhStack, P.two_level ? kBvh4Stack : 0);
    const BvhBuild& B = fit.bvh;
    if (B.depth >= kBvhStack) return set_err(c, XRT_ERR_UNSUPPORTED, "BVH deeper than the traversal stack");
    std::vector<f4> btri(3 * nt);
    for (size_t i = 0; i < nt; ++i) {
        const uint32_t t = big[B.order[i]];
        btri[3 * i] = tri[3 * t], btri[3 * i + 1] = tri[3 * t + 1], btri[3 * i + 2] = tri[3 * t + 2];
        btri[3 * i + 2].w = bits((int)t);
    }
    if ((rc = upload(c, c->bvh_node, B.nodes.data(), B.nodes.size() * sizeof(BvhNode))) ||
        (rc = upload(c, c->bvh_tri, btri.data(), btri.size() * sizeof(f4))))
        return rc;
    P.bvh_node = as<f4>(c->bvh_node), P.bvh_tri = as<f4>(c->bvh_tri);
    P.bvh_stack = B.depth + 1;
    P.bvh_nodes = (int)B.nodes.size();
    c->bvh_tris = (int)nt;
    if (P.two_level) {   // the deep rays walk the 4-wide form
        const int d4 = fit.depth4;
        const std::vector<Bvh4Node>& b4 = fit.bvh4;
        if (3 * d4 + 1 > kBvh4Stack) return set_err(c, XRT_ERR_UNSUPPORTED, "4-wide BVH deeper than the traversal stack");
        if ((rc = upload(c, c->bvh4, b4.data(), b4.size() * sizeof(Bvh4Node)))) return rc;
        P.bvh4 = as<f4>(c->bvh4), P.bvh4_nodes = (int)b4.size(), P.bvh4_stack = 3 * d4 + 1;
    }
    return XRT_OK;
}

// sphere scenes (C3's 1001 spheres): a threaded BVH for the fused schedule's traces.
// Sphere boxes: center +- radius, padded by 1e-4 — far above the float error of
// Sphere::intersect's hit point (and of its near-tangent discriminant).
int build_sphere_bvh(xrt_ctx* c, const FlatScene& F) {
    KParams& P = c->base;
    P.snode = nullptr, P.ssph = nullptr, P.sbk = nullptr, P.sblk = nullptr, P.n_snode = 0, P.sph_pad = 0.0f;
    if (!(P.scene_kind == SCN_SPHERE && P.n_sph >= kSphBvhMin && !exp_env("XRT_NO_BVH"))) return XRT_OK;
    const std::vector<f4>& sph = F.sph;
    const size_t ns = (size_t)P.n_sph;
    std::vector<float> mn(3 * ns), mx(3 * ns);
    Bounds scene;
    for (size_t k = 0; k < ns; ++k) {
        const float cc[3] = {sph[k].x, sph[k].y, sph[k].z}, r = std::fabs(sph[k].w);
        for (int q = 0; q < 3; ++q) mn[3 * k + q] = cc[q] - r, mx[3 * k + q] = cc[q] + r;
        scene.grow(&mn[3 * k], &mx[3 * k]);
    }
    P.sph_pad = scene.pad(1e-4f);
    const BvhBuild B = build_bvh(mn.data(), mx.data(), (uint32_t)ns, kBvhLeaf, P.sph_pad, kBvhMaxDepth);
    const std::vector<SkipNode> T = thread_bvh(B);
    std::vector<f4> bs(ns);
    std::vector<int> bk(ns);
    for (size_t i = 0; i < ns; ++i) {
        const uint32_t k = B.order[i];
        bs[i] = sph[k];
        bk[i] = (int)k | (F.sph_obj[k] & (1 << 30));
    }
    // a ball around every 64 consecutive spheres of the leaf order (spatially coherent
    // blocks): it contains each member's ball of radius |r| + sph_pad, so the pixel
    // schedule's list scans skip a block whose ball misses the region (pixel.hip)
    std::vector<f4> blk((ns + 63) / 64);
    for (size_t b = 0; b < blk.size(); ++b) {
        const size_t i0 = 64 * b, i1 = std::min(ns, i0 + 64);
        double lo3[3] = {1e300, 1e300, 1e300}, hi3[3] = {-1e300, -1e300, -1e300};
        for (size_t i = i0; i < i1; ++i)
            for (int q = 0; q < 3; ++q) {
                const double cq = q == 0 ? bs[i].x : q == 1 ? bs[i].y : bs[i].z;
                lo3[q] = std::min(lo3[q], cq), hi3[q] = std::max(hi3[q], cq);
            }
        const double C[3] = {0.5 * (lo3[0] + hi3[0]), 0.5 * (lo3[1] + hi3[1]), 0.5 * (lo3[2] + hi3[2])};
        const float Cf[3] = {(float)C[0], (float)C[1], (float)C[2]};
        double R = 0.0;
        for (size_t i = i0; i < i1; ++i) {
            const double dx = (double)bs[i].x - Cf[0], dy = (double)bs[i].y - Cf[1], dz = (double)bs[i].z - Cf[2];
            R = std::max(R, std::sqrt(dx * dx + dy * dy + dz * dz) + std::fabs((double)bs[i].w));
        }
        blk[b] = f4{Cf[0], Cf[1], Cf[2], (float)(R * (1.0 + 1e-5)) + P.sph_pad};
    }
    int rc;
    if ((rc = upload(c, c->snode, T.data(), T.size() * sizeof(SkipNode))) ||
        (rc = upload(c, c->ssph, bs.data(), bs.size() * sizeof(f4))) ||
        (rc = upload(c, c->sbk, bk.data(), bk.size() * sizeof(int))) ||
        (rc = upload(c, c->sblk, blk.data(), blk.size() * sizeof(f4))))
        return rc;
    P.snode = as<f4>(c->snode), P.ssph = as<f4>(c->ssph), P.sbk = as<int>(c->sbk);
    P.sblk = as<f4>(c->sblk);
    P.n_snode = (int)T.size();
    return XRT_OK;
}

int upload_scene_one(xrt_ctx* c, const xrt_scene_desc* s) {
    if (!c || !s) return XRT_ERR_INVALID;
    // a failed upload (OOM, bad range) must not leave the previous scene's freed buffers
    // behind a valid-looking context: renders are refused until an upload completes
    c->has_scene = false;
    HIPCHK(c, hipSetDevice(c->device));
    FlatScene F;
    int rc;
    if ((rc = flatten_scene(c, s, F)) || (rc = upload_flat(c, F)) || (rc = build_small_scene(c, F)) ||
        (rc = build_tri_bvh(c, F)) || (rc = build_sphere_bvh(c, F)))
        return rc;
    c->obj_tri_first = std::move(F.tri_first);
    c->has_mirror = F.has_mirror, c->has_glass = F.has_glass;   // the flags change only when the upload succeeds
    c->has_scene = true;
    return XRT_OK;
}

int set_camera_one(xrt_ctx* c, const float c2w[16], float scale, float aspect) {
    if (!c || !c2w) return XRT_ERR_INVALID;
    std::memcpy(c->base.c2w, c2w, sizeof(float) * 16);
    c->base.scale = scale;
    c->base.aspect = aspect;
    c->has_camera = true;
    return XRT_OK;
}

// DeltaLight::sample returns color * intensity (Src/light.cpp:127,141): multiplied once here,
// the same float product
int set_delta_lights_one(xrt_ctx* c, const xrt_delta_light* lights, uint32_t n) {
    if (!c || (n && !lights)) return XRT_ERR_INVALID;
    if (n > XRT_MAX_DELTA_LIGHTS)
        return set_err(c, XRT_ERR_UNSUPPORTED, "more than " + std::to_string(XRT_MAX_DELTA_LIGHTS) + " delta lights");
    std::vector<DDelta> d(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (lights[i].kind != XRT_DLIGHT_POINT && lights[i].kind != XRT_DLIGHT_DISTANT)
            return set_err(c, XRT_ERR_INVALID, "delta light " + std::to_string(i) + ": unknown kind");
        d[i].kind = lights[i].kind;
        for (int q = 0; q < 3; ++q) {
            d[i].pos[q] = lights[i].pos[q], d[i].dir[q] = lights[i].dir[q];
            d[i].L[q] = lights[i].color[q] * lights[i].intensity;
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = upload(c, c->dlights, d.data(), n * sizeof(DDelta));
    if (rc) return rc;
    c->base.dlights = as<DDelta>(c->dlights);
    c->base.n_dlights = (int)n;
    return XRT_OK;
}

// the grid-independent part of a heterogeneous medium (dense or bricks)
int set_medium_grid(xrt_ctx* c, const xrt_medium_desc* m) {
    DMedium& D = c->base.medium;
    D.nx = (int)m->nx, D.ny = (int)m->ny, D.nz = (int)m->nz;
    for (int q = 0; q < 3; ++q) {
        D.origin[q] = m->origin[q];
        D.absorption[q] = m->absorption[q];
        D.scattering[q] = m->scattering[q];
    }
    D.voxel_size = m->voxel_size;
    D.inv_voxel = 1.0 / (double)m->voxel_size;
    D.multiplier = m->density_multiplier;
    D.g = m->g;
    D.kind = XRT_MEDIUM_HETEROGENEOUS;
    // HeterogeneousMedium ctor (Src/medium.cpp:5-17)
    const float max_density = m->density_multiplier * m->max_density;
    const Vec3f a(m->absorption[0], m->absorption[1], m->absorption[2]);
    const Vec3f sc(m->scattering[0], m->scattering[1], m->scattering[2]);
    const Vec3f mm = a * max_density + sc * max_density;
    D.majorant = std::max(mm[0], std::max(mm[1], mm[2]));
    D.inv_majorant = 1.0f / D.majorant;
    c->has_medium = true;
    return XRT_OK;
}

int set_medium_one(xrt_ctx* c, const xrt_medium_desc* m) {
    if (!c || !m) return XRT_ERR_INVALID;
    if (m->kind != XRT_MEDIUM_HETEROGENEOUS) {
        // HomogeneousMedium{MIS, Achromatic, NoMIS} (Src/medium.h:122-277): sigma_t = a + s
        if (m->kind > XRT_MEDIUM_HOMOGENEOUS_NOMIS || m->kind < 0) return set_err(c, XRT_ERR_INVALID, "bad medium kind");
        DMedium& D = c->base.medium;
        D = DMedium{};
        D.kind = m->kind;
        D.g = m->g;
        const Vec3f a(m->absorption[0], m->absorption[1], m->absorption[2]);
        const Vec3f sc(m->scattering[0], m->scattering[1], m->scattering[2]);
        const Vec3f t = a + sc;
        for (int q = 0; q < 3; ++q) D.absorption[q] = a[q], D.scattering[q] = sc[q], D.sigma_t[q] = t[q];
        c->has_medium = true;
        return XRT_OK;
    }
    if (!m->density || !m->nx || !m->ny || !m->nz) return XRT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)m->nx * m->ny * m->nz;
    int rc = upload(c, c->density, m->density, n * sizeof(float));
    if (rc) return rc;
    DMedium& D = c->base.medium;
    D = DMedium{};
    D.density = as<float>(c->density);
    // the per-cell corner layout (8x the grid's bytes; skipped above the context's limit, 2 GiB
    // unless a test set another with xrt_test_corner_grid_limit).  It is only an
    // acceleration: when the host copy or the device buffer cannot be had, the medium reads
    // the dense grid's rows instead (D.corners = null), with identical results.
    const size_t cx = m->nx - 1, cy = m->ny - 1, cz = m->nz - 1, cells = cx * cy * cz;
    free_buf(c->corners);
    if (XRT_CORNER_GRID && cells && cells * 32 <= c->corner_limit) {
        std::vector<float> cor;
        try {
            cor.resize(cells * 8);
        } catch (const std::bad_alloc&) {
            cor.clear();
        }
        if (!cor.empty()) {
            const float* g = m->density;
            const size_t sy = m->nx, sz = (size_t)m->nx * m->ny;
            for (size_t k = 0; k < cz; ++k)
                for (size_t j = 0; j < cy; ++j)
                    for (size_t i = 0; i < cx; ++i) {
                        const float* b = g + k * sz + j * sy + i;
                        float* o = cor.data() + 8 * ((k * cy + j) * cx + i);
                        o[0] = b[0], o[1] = b[sz], o[2] = b[sy], o[3] = b[sy + sz];
                        o[4] = b[1], o[5] = b[1 + sz], o[6] = b[1 + sy], o[7] = b[1 + sy + sz];
                    }
            if (upload(c, c->corners, cor.data(), cor.size() * sizeof(float)) == XRT_OK) {
                D.corners = as<float>(c->corners);
            } else {
                free_buf(c->corners);
                (void)hipGetLastError();
                c->err.clear();
            }
        }
    }
    return set_medium_grid(c, m);
}

// Sparse heterogeneous density in XRT_BRICK^3 leaf bricks (the NanoVDB / OpenVDB leaf
// layout): the same trilinear BoxSampler as the dense grid, reading voxels through the brick
// table (medium_density), so inactive regions cost no memory.
int set_medium_bricks_one(xrt_ctx* c, const xrt_medium_desc* m, const xrt_brick_grid* g) {
    if (!c || !m || !g) return XRT_ERR_INVALID;
    if (m->kind != XRT_MEDIUM_HETEROGENEOUS) return set_err(c, XRT_ERR_INVALID, "brick grids are heterogeneous media");
    if (!m->nx || !m->ny || !m->nz || !g->table || (g->n_bricks && !g->bricks) || g->nbx != (m->nx + 7) / 8 ||
        g->nby != (m->ny + 7) / 8 || g->nbz != (m->nz + 7) / 8)
        return set_err(c, XRT_ERR_INVALID, "brick table dimensions do not match the grid (ceil(n / 8) per axis)");
    const size_t nt = (size_t)g->nbx * g->nby * g->nbz;
    for (size_t i = 0; i < nt; ++i)
        if (g->table[i] < -1 || g->table[i] >= (int32_t)g->n_bricks)
            return set_err(c, XRT_ERR_INVALID, "brick table entry out of range");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = upload(c, c->brick_table, g->table, nt * sizeof(int32_t))) ||
        (rc = upload(c, c->brick_data, g->bricks, (size_t)g->n_bricks * 512 * sizeof(float))))
        return rc;
    DMedium& D = c->base.medium;
    D = DMedium{};
    D.brick_table = as<int>(c->brick_table);
    D.bricks = as<float>(c->brick_data);
    D.nbx = (int)g->nbx, D.nby = (int)g->nby, D.nbz = (int)g->nbz;
    return set_medium_grid(c, m);
}

}  // namespace

extern "C" {

int xrt_upload_scene(xrt_ctx* c, const xrt_scene_desc* s) {
    end_progressive(c);   // an open progressive session renders what was set before
    return for_each_device(c, "xrt_upload_scene", [&](xrt_ctx* d) { return upload_scene_one(d, s); });
}

int xrt_set_camera(xrt_ctx* c, const float c2w[16], float scale, float aspect) {
    end_progressive(c);   // an open progressive session renders what was set before
    return for_each_device(c, "xrt_set_camera", [&](xrt_ctx* d) { return set_camera_one(d, c2w, scale, aspect); });
}

int xrt_set_delta_lights(xrt_ctx* c, const xrt_delta_light* lights, uint32_t n) {
    end_progressive(c);   // an open progressive session renders what was set before
    return for_each_device(c, "xrt_set_delta_lights", [&](xrt_ctx* d) { return set_delta_lights_one(d, lights, n); });
}

int xrt_set_medium(xrt_ctx* c, const xrt_medium_desc* m) {
    end_progressive(c);   // an open progressive session renders what was set before
    return for_each_device(c, "xrt_set_medium", [&](xrt_ctx* d) { return set_medium_one(d, m); });
}

int xrt_set_medium_bricks(xrt_ctx* c, const xrt_medium_desc* m, const xrt_brick_grid* g) {
    end_progressive(c);   // an open progressive session renders what was set before
    return for_each_device(c, "xrt_set_medium_bricks", [&](xrt_ctx* d) { return set_medium_bricks_one(d, m, g); });
}

// a self-test's knob: where set_medium_one stops building the corner values, on every device
int xrt_test_corner_grid_limit(xrt_ctx* c, uint64_t max_bytes) {
    return for_each_device(c, "xrt_test_corner_grid_limit", [&](xrt_ctx* d) {
        if (!d) return (int)XRT_ERR_INVALID;
        d->corner_limit = (size_t)max_bytes;
        return (int)XRT_OK;
    });
}

}  // extern "C"
