// api_aov.cpp — the C ABI of include/xrt.h, the first-hit guide buffers (the filters that read
// them: api_denoise.cpp).
#include <chrono>

#include "ctx.h"

using namespace xrt;

// ------------------------------------------------------------ guide buffers ----
// xrt_render_aov / xrt_render_aov_device (aov.hip).  The plan has the pixel schedule's shape
// without its ends: k_seed, one k_aov / k_aov_bvh launch that divides and writes its planes
// itself, no live lists, no k_finish.  The five planes are handled as an array in
// xrt_aov_buffers' member order; each element is 4 bytes.
static constexpr int kAovPlanes = 5;
static constexpr size_t kAovCh[kAovPlanes] = {3, 3, 1, 1, 1};   // elements per pixel

static void aov_ptrs(const xrt_aov_buffers& b, void* q[kAovPlanes]) {
    q[0] = b.albedo, q[1] = b.normal, q[2] = b.depth, q[3] = b.alpha, q[4] = b.object;
}

static int aov_check(xrt_ctx* c, const xrt_render_params* p, const xrt_aov_buffers* out) {
    if (!c || !p || !out) return set_err(c, XRT_ERR_INVALID, "xrt_render_aov: null argument");
    if (!out->albedo && !out->normal && !out->depth && !out->alpha && !out->object)
        return set_err(c, XRT_ERR_INVALID, "xrt_render_aov: no plane requested (all five buffers are NULL)");
    if (p->width == 0 || p->height == 0 || p->shard_count == 0 || p->shard_index >= p->shard_count)
        return set_err(c, XRT_ERR_INVALID, "bad image size or shard");
    if (p->spp == 0) return set_err(c, XRT_ERR_INVALID, "xrt_render_aov: spp must be positive");
    if (p->flags & XRT_FLAG_ACCUMULATE)
        return set_err(c, XRT_ERR_UNSUPPORTED, "xrt_render_aov: XRT_FLAG_ACCUMULATE (guide buffers are not accumulated)");
    return XRT_OK;
}

// the context's own planes for the wanted ones: [npix] x (3 + 3 + 1 + 1 + 1) elements
static int aov_own(xrt_ctx* c, size_t npix, const xrt_aov_buffers& want, xrt_aov_buffers& own) {
    const int rc = ensure(c, c->aov, 9 * npix * sizeof(float));
    if (rc) return rc;
    float* b = as<float>(c->aov);
    own.albedo = want.albedo ? b : nullptr;
    own.normal = want.normal ? b + 3 * npix : nullptr;
    own.depth = want.depth ? b + 6 * npix : nullptr;
    own.alpha = want.alpha ? b + 7 * npix : nullptr;
    own.object = want.object ? reinterpret_cast<int32_t*>(b + 8 * npix) : nullptr;
    return XRT_OK;
}

static int aov_copy_out(xrt_ctx* c, size_t npix, const xrt_aov_buffers& host, const xrt_aov_buffers& dev) {
    void *h[kAovPlanes], *d[kAovPlanes];
    aov_ptrs(host, h), aov_ptrs(dev, d);
    for (int k = 0; k < kAovPlanes; ++k)
        if (h[k]) HIPCHK(c, hipMemcpy(h[k], d[k], npix * kAovCh[k] * 4, hipMemcpyDeviceToHost));
    return XRT_OK;
}

// one device: the planes of `out` (device pointers on c's GPU; null = not wanted).
// wait: 0 = none, 2 = the caller's stream `wait_stream` (xrt_render_device_after's ordering)
static int aov_one(xrt_ctx* c, const xrt_render_params* p, const xrt_aov_buffers& out, xrt_stats* st, int wait,
                   hipStream_t wait_stream) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!c->has_scene || !c->has_camera) return set_err(c, XRT_ERR_STATE, "upload a scene and set a camera first");
    end_progressive(c);   // k_seed below resets the slots
    int rc = order_after(c, wait, wait_stream, false);
    if (rc) return rc;
    const size_t n = (size_t)shard_rows(p->height, p->shard_index, p->shard_count) * p->width;
    const size_t npix = (size_t)p->width * p->height;
    if (n && (rc = grow_slots(c, n))) return rc;
    KParams P = render_params(c, p, n, nullptr);
    if (!aov_kernel(P))
        return set_err(c, XRT_ERR_UNSUPPORTED,
                       "xrt_render_aov: the scene neither fits the LDS-resident scene carve nor has a triangle BVH "
                       "(a large sphere-only or mixed scene)");
    // pixels outside the shard: 0, object -1
    void* q[kAovPlanes];
    aov_ptrs(out, q);
    for (int k = 0; k < kAovPlanes; ++k)
        if (q[k]) HIPCHK(c, hipMemsetAsync(q[k], k == 4 ? 0xff : 0, npix * kAovCh[k] * 4, c->stream));
    xrt_stats S{};
    S.schedule = XRT_SCHED_AOV;
    LaunchTimer T{c, S, (p->flags & XRT_FLAG_TIMING) != 0, {}, {}};
    if (n) {
        // k_seed's lists: one partition holding every slot
        P.n_part = 1, P.part_cap = (uint32_t)n, P.rng_keep = 0;
        const LiveLists L{{as<uint32_t>(c->lists), as<uint32_t>(c->lists) + n}, as<uint32_t>(c->counts)};
        P.req = as<uint32_t>(c->lists) + 2 * n;
        S.path_slots = n;
        S.samples = (uint64_t)n * p->spp;
        HIPCHK(c, hipMemsetAsync(P.stats, 0, 512, c->stream));
        HIPCHK(c, T.launch(XRT_K_SEED, [&] { return launch_seed(P, L.list[0], L.counts(0), L.counts(1), L.req(0), c->stream); }));
        const AovOut A{out.albedo, out.normal, out.depth, out.alpha, out.object, as<float>(c->obj_albedo)};
        uint32_t* work = reinterpret_cast<uint32_t*>(P.stats + kStatsWork);   // the pixel counter: a stats word
        const hipError_t e = T.launch(XRT_K_STEP, [&] { return launch_aov(P, A, work, c->stream); });
        if (e != hipSuccess) return hip_err(c, e, aov_kernel(P) == 2 ? "k_aov_bvh" : "k_aov");
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // one Scene::intersect and two draws per sample; the stream is generated in LDS, as many
    // 624-word blocks per pixel as a std::mt19937 twists for 2 spp words
    S.segments = S.samples, S.draws = 2 * S.samples;
    S.rng_twists = S.path_slots * ((2ull * p->spp + kMT - 1) / kMT);
    T.read_out();
    S.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (st) *st = S;
    return XRT_OK;
}

// d_out: the caller's device planes on subs[0]'s GPU, or null: host planes h_out
static int aov_multi(xrt_ctx* m, const xrt_render_params* p, const xrt_aov_buffers* d_out, const xrt_aov_buffers* h_out,
                     xrt_stats* st, int wait, hipStream_t wait_stream) {
    const auto t_start = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)m->subs.size();
    const size_t npix = (size_t)p->width * p->height;
    const xrt_aov_buffers& want = d_out ? *d_out : *h_out;
    xrt_ctx* s0 = m->subs[0];
    int rc = order_after(s0, wait, wait_stream, true);
    if (rc) return set_err(m, rc, s0->err);
    // every device renders into its own planes; device 0 directly into the caller's
    std::vector<xrt_aov_buffers> bufs(n);
    std::vector<RowPlane> planes(kAovPlanes);
    for (uint32_t i = 0; i < n; ++i) {
        xrt_ctx* s = m->subs[i];
        HIPCHK(m, hipSetDevice(s->device));
        if (i == 0 && d_out)
            bufs[0] = *d_out;
        else if ((rc = aov_own(s, npix, want, bufs[i])))
            return multi_fail(m, s, rc, "guide buffers");
        void* q[kAovPlanes];
        aov_ptrs(bufs[i], q);
        for (int k = 0; k < kAovPlanes; ++k) planes[k].dev.push_back(q[k]), planes[k].pixel_bytes = kAovCh[k] * 4;
    }
    std::vector<xrt_stats> S(n);
    if ((rc = fan_out_rows(m, p, "xrt_render_aov",
                           [&](uint32_t i, const xrt_render_params* q) {
                               return aov_one(m->subs[i], q, bufs[i], &S[i], 0, nullptr);
                           })) ||
        (rc = gather_rows(m, p, planes)))
        return rc;
    if (h_out && (rc = aov_copy_out(s0, npix, *h_out, bufs[0]))) return multi_fail(m, s0, rc, "xrt_render_aov");
    if (st) {
        *st = sum_stats(S);
        st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return XRT_OK;
}

extern "C" {

int xrt_render_aov(xrt_ctx* c, const xrt_render_params* p, const xrt_aov_buffers* host_out, xrt_stats* st) {
    const auto t_start = std::chrono::steady_clock::now();
    int rc = aov_check(c, p, host_out);
    if (rc) return rc;
    if (!c->subs.empty()) return aov_multi(c, p, nullptr, host_out, st, 0, nullptr);
    const size_t npix = (size_t)p->width * p->height;
    xrt_aov_buffers own;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = aov_own(c, npix, *host_out, own)) || (rc = aov_one(c, p, own, st, 0, nullptr)) ||
        (rc = aov_copy_out(c, npix, *host_out, own)))
        return rc;
    if (st) st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return XRT_OK;
}

int xrt_render_aov_device(xrt_ctx* c, const xrt_render_params* p, const xrt_aov_buffers* device_out, void* hip_stream,
                          xrt_stats* st) {
    const int rc = aov_check(c, p, device_out);
    if (rc) return rc;
    if (!c->subs.empty()) return aov_multi(c, p, device_out, nullptr, st, 2, (hipStream_t)hip_stream);
    return aov_one(c, p, *device_out, st, 2, (hipStream_t)hip_stream);
}

}  // extern "C"
