// api_aov.cpp — the C ABI of include/xrt.h, the first-hit guide buffers and the denoiser that
// reads them.
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

// ------------------------------------------------------------------ denoiser ----
// xrt_denoise / xrt_denoise_device (denoise.hip): the prepass packs the planes into records, then
// one launch per iteration, ping-ponging the colour records; the last writes `out`.
// host: color / guides / out are host memory, staged through the context's buffer.
// wait_stream: the device entry point's ordering (xrt_render_aov_device's).
static int denoise_impl(xrt_ctx* m, const xrt_denoise_params* p, const float* color, const xrt_aov_buffers* guides,
                        float* out, bool host, hipStream_t wait_stream, xrt_denoise_stats* st) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!m || !p || !out) return set_err(m, XRT_ERR_INVALID, "xrt_denoise: null argument");
    if (p->width == 0 || p->height == 0) return set_err(m, XRT_ERR_INVALID, "xrt_denoise: bad image size");
    if (p->iterations == 0 || p->iterations > XRT_DENOISE_MAX_ITERATIONS)
        return set_err(m, XRT_ERR_INVALID, "xrt_denoise: iterations must be 1 .. XRT_DENOISE_MAX_ITERATIONS");
    xrt_ctx* c = first_device(m);
    auto fail = [&](int rc) { return c == m ? rc : multi_fail(m, c, rc, "xrt_denoise"); };
    const size_t npix = (size_t)p->width * p->height;
    if (!color && (!c->fb.p || npix * 3 * sizeof(float) > c->fb.bytes))
        return set_err(m, XRT_ERR_STATE, "xrt_denoise: no framebuffer of that size (render first)");
    int rc = order_after(c, host ? 0 : 2, wait_stream, false);
    if (rc) return set_err(m, rc, c->err);
    const xrt_aov_buffers none{nullptr, nullptr, nullptr, nullptr, nullptr};
    const xrt_aov_buffers& g = guides ? *guides : none;
    // records: col[2], nrm, alb; host staging behind them: color 3, albedo 3, normal 3, depth 1, object 1, out 3
    if ((rc = ensure(c, c->denoise, npix * (4 * sizeof(f4) + (host ? 14 * sizeof(float) : 0))))) return fail(rc);
    f4* rec = as<f4>(c->denoise);
    f4 *col[2] = {rec, rec + npix}, *nrm = rec + 2 * npix, *alb = rec + 3 * npix;
    const float* d_color = color ? color : as<float>(c->fb);
    const float *d_albedo = g.albedo, *d_normal = g.normal, *d_depth = g.depth;
    const int32_t* d_object = g.object;
    float* d_out = out;
    if (host) {
        float* s = reinterpret_cast<float*>(rec + 4 * npix);
        auto stage = [&](const void* src, size_t off, size_t ch) -> const float* {
            if (!src) return nullptr;
            return hipMemcpyAsync(s + off * npix, src, npix * ch * 4, hipMemcpyHostToDevice, c->stream) == hipSuccess
                       ? s + off * npix : nullptr;
        };
        if (color && !(d_color = stage(color, 0, 3))) return fail(set_err(c, XRT_ERR_HIP, "xrt_denoise: copy of color"));
        d_albedo = stage(g.albedo, 3, 3), d_normal = stage(g.normal, 6, 3), d_depth = stage(g.depth, 9, 1);
        d_object = reinterpret_cast<const int32_t*>(stage(g.object, 10, 1));
        if ((g.albedo && !d_albedo) || (g.normal && !d_normal) || (g.depth && !d_depth) || (g.object && !d_object))
            return fail(set_err(c, XRT_ERR_HIP, "xrt_denoise: copy of a guide plane"));
        d_out = s + 11 * npix;
    }
    const float sig[4] = {p->sigma_color, p->sigma_normal, p->sigma_depth, p->sigma_albedo};
    float inv[4];
    for (int k = 0; k < 4; ++k) inv[k] = sig[k] > 0.0f ? 1.0f / (sig[k] * sig[k]) : 0.0f;
    xrt_stats S{};
    xrt_denoise_stats D{};
    LaunchTimer T{c, S, (p->flags & XRT_DENOISE_TIMING) != 0, {}, {}};
    hipError_t e = T.launch(XRT_K_STEP, [&] {
        return launch_denoise_pack(d_color, d_albedo, d_normal, d_depth, d_object, npix, col[0], nrm, alb, c->stream);
    });
    if (e != hipSuccess) return fail(hip_err(c, e, "k_dn_pack"));
    for (uint32_t i = 0; i < p->iterations; ++i) {
        const float scale = (float)(1u << (2 * i));
        const bool last = i + 1 == p->iterations;
        const bool tiled = !(p->flags & XRT_DENOISE_NO_TILE) && i < XRT_DENOISE_TILED_ITERATIONS && denoise_has_tiled(1 << i);
        const DenoiseIter I{col[i & 1], nrm, alb, last ? nullptr : col[(i + 1) & 1], last ? d_out : nullptr,
                            p->width, p->height, 1 << i, DenoiseK{inv[0] * scale, inv[1], inv[2] * (1.0f / scale), inv[3]}};
        e = T.launch(XRT_K_STEP, [&] { return launch_denoise_iter(I, tiled, c->stream); });
        if (e != hipSuccess) return fail(hip_err(c, e, tiled ? "k_dn_tiled" : "k_dn_direct"));
        (tiled ? D.tiled_iterations : D.direct_iterations)++;
    }
    if (host) e = hipMemcpyAsync(out, d_out, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(hip_err(c, e, "xrt_denoise"));
    T.read_out();
    D.kernel_ms = S.kernel_ms[XRT_K_STEP];
    D.launches = (uint32_t)S.launches[XRT_K_STEP];
    D.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (st) *st = D;
    return XRT_OK;
}

// xrt_denoise_var / xrt_denoise_var_device (denoise_var.hip): denoise_impl's shape with the variance
// carried in the colour records.  The prepass packs into col[0]; without a caller's variance it
// packs into col[1] and the estimate writes col[0] = {rgb, estimate} from it.
static int denoise_var_impl(xrt_ctx* m, const xrt_denoise_var_params* p, const float* color, const float* variance,
                            const xrt_aov_buffers* guides, float* out, float* out_variance, bool host, hipStream_t wait_stream,
                            xrt_denoise_stats* st) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!m || !p || !out) return set_err(m, XRT_ERR_INVALID, "xrt_denoise_var: null argument");
    if (p->width == 0 || p->height == 0) return set_err(m, XRT_ERR_INVALID, "xrt_denoise_var: bad image size");
    if (p->iterations == 0 || p->iterations > XRT_DENOISE_MAX_ITERATIONS)
        return set_err(m, XRT_ERR_INVALID, "xrt_denoise_var: iterations must be 1 .. XRT_DENOISE_MAX_ITERATIONS");
    if (!variance && (p->variance_radius < 1 || p->variance_radius > XRT_DENOISE_VAR_MAX_RADIUS))
        return set_err(m, XRT_ERR_INVALID, "xrt_denoise_var: variance_radius must be 1 .. XRT_DENOISE_VAR_MAX_RADIUS without a variance plane");
    xrt_ctx* c = first_device(m);
    auto fail = [&](int rc) { return c == m ? rc : multi_fail(m, c, rc, "xrt_denoise_var"); };
    const size_t npix = (size_t)p->width * p->height;
    if (!color && (!c->fb.p || npix * 3 * sizeof(float) > c->fb.bytes))
        return set_err(m, XRT_ERR_STATE, "xrt_denoise_var: no framebuffer of that size (render first)");
    int rc = order_after(c, host ? 0 : 2, wait_stream, false);
    if (rc) return set_err(m, rc, c->err);
    const xrt_aov_buffers none{nullptr, nullptr, nullptr, nullptr, nullptr};
    const xrt_aov_buffers& g = guides ? *guides : none;
    // records: col[2], nrm, alb; host staging behind them: color 3, albedo 3, normal 3, depth 1, object 1,
    // variance 1, out 3, out_variance 1
    if ((rc = ensure(c, c->denoise, npix * (4 * sizeof(f4) + (host ? 16 * sizeof(float) : 0))))) return fail(rc);
    f4* rec = as<f4>(c->denoise);
    f4 *col[2] = {rec, rec + npix}, *nrm = rec + 2 * npix, *alb = rec + 3 * npix;
    const float* d_color = color ? color : as<float>(c->fb);
    const float *d_variance = variance, *d_albedo = g.albedo, *d_normal = g.normal, *d_depth = g.depth;
    const int32_t* d_object = g.object;
    float *d_out = out, *d_outv = out_variance;
    if (host) {
        float* s = reinterpret_cast<float*>(rec + 4 * npix);
        auto stage = [&](const void* src, size_t off, size_t ch) -> const float* {
            if (!src) return nullptr;
            return hipMemcpyAsync(s + off * npix, src, npix * ch * 4, hipMemcpyHostToDevice, c->stream) == hipSuccess
                       ? s + off * npix : nullptr;
        };
        if (color && !(d_color = stage(color, 0, 3))) return fail(set_err(c, XRT_ERR_HIP, "xrt_denoise_var: copy of color"));
        d_albedo = stage(g.albedo, 3, 3), d_normal = stage(g.normal, 6, 3), d_depth = stage(g.depth, 9, 1);
        d_object = reinterpret_cast<const int32_t*>(stage(g.object, 10, 1));
        d_variance = stage(variance, 11, 1);
        if ((g.albedo && !d_albedo) || (g.normal && !d_normal) || (g.depth && !d_depth) || (g.object && !d_object) ||
            (variance && !d_variance))
            return fail(set_err(c, XRT_ERR_HIP, "xrt_denoise_var: copy of a guide or variance plane"));
        d_out = s + 12 * npix;
        d_outv = out_variance ? s + 15 * npix : nullptr;
    }
    const float sig[3] = {p->sigma_normal, p->sigma_depth, p->sigma_albedo};
    float inv[3];
    for (int k = 0; k < 3; ++k) inv[k] = sig[k] > 0.0f ? 1.0f / (sig[k] * sig[k]) : 0.0f;
    xrt_stats S{};
    xrt_denoise_stats D{};
    LaunchTimer T{c, S, (p->flags & XRT_DENOISE_TIMING) != 0, {}, {}};
    hipError_t e = T.launch(XRT_K_STEP, [&] {
        return launch_dnv_pack(d_color, d_variance, d_albedo, d_normal, d_depth, d_object, npix, col[variance ? 0 : 1], nrm, alb,
                               c->stream);
    });
    if (e != hipSuccess) return fail(hip_err(c, e, "k_dnv_pack"));
    if (!variance) {
        e = T.launch(XRT_K_STEP, [&] {
            return launch_dnv_estimate(col[1], nrm, col[0], p->width, p->height, (int)p->variance_radius, c->stream);
        });
        if (e != hipSuccess) return fail(hip_err(c, e, "k_dnv_estimate"));
    }
    for (uint32_t i = 0; i < p->iterations; ++i) {
        const float scale = (float)(1u << (2 * i));
        const bool last = i + 1 == p->iterations;
        const bool tiled = !(p->flags & XRT_DENOISE_NO_TILE) && i < XRT_DENOISE_VAR_TILED_ITERATIONS && dnv_has_tiled(1 << i);
        const DnvIter I{col[i & 1], nrm, alb, last ? nullptr : col[(i + 1) & 1], last ? d_out : nullptr, last ? d_outv : nullptr,
                        p->width, p->height, 1 << i, DnvK{p->sigma_luminance, inv[0], inv[1] * (1.0f / scale), inv[2]}};
        e = T.launch(XRT_K_STEP, [&] { return launch_dnv_iter(I, tiled, c->stream); });
        if (e != hipSuccess) return fail(hip_err(c, e, tiled ? "k_dnv_tiled" : "k_dnv_direct"));
        (tiled ? D.tiled_iterations : D.direct_iterations)++;
    }
    if (host) {
        e = hipMemcpyAsync(out, d_out, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && out_variance)
            e = hipMemcpyAsync(out_variance, d_outv, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(hip_err(c, e, "xrt_denoise_var"));
    T.read_out();
    D.kernel_ms = S.kernel_ms[XRT_K_STEP];
    D.launches = (uint32_t)S.launches[XRT_K_STEP];
    D.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (st) *st = D;
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

int xrt_denoise(xrt_ctx* c, const xrt_denoise_params* p, const float* color, const xrt_aov_buffers* guides, float* out,
                xrt_denoise_stats* st) {
    return denoise_impl(c, p, color, guides, out, true, nullptr, st);
}

int xrt_denoise_device(xrt_ctx* c, const xrt_denoise_params* p, const float* d_color, const xrt_aov_buffers* d_guides,
                       float* d_out, void* hip_stream, xrt_denoise_stats* st) {
    return denoise_impl(c, p, d_color, d_guides, d_out, false, (hipStream_t)hip_stream, st);
}

int xrt_denoise_var(xrt_ctx* c, const xrt_denoise_var_params* p, const float* color, const float* variance,
                    const xrt_aov_buffers* guides, float* out, float* out_variance, xrt_denoise_stats* st) {
    return denoise_var_impl(c, p, color, variance, guides, out, out_variance, true, nullptr, st);
}

int xrt_denoise_var_device(xrt_ctx* c, const xrt_denoise_var_params* p, const float* d_color, const float* d_variance,
                           const xrt_aov_buffers* d_guides, float* d_out, float* d_out_variance, void* hip_stream,
                           xrt_denoise_stats* st) {
    return denoise_var_impl(c, p, d_color, d_variance, d_guides, d_out, d_out_variance, false, (hipStream_t)hip_stream, st);
}

}  // extern "C"
