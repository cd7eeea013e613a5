// api_denoise.cpp — the C ABI of include/xrt.h, the two a-trous filters over a frame and its guide
// buffers: xrt_denoise / xrt_denoise_device and xrt_denoise_var / xrt_denoise_var_device (denoise.hip).
#include <chrono>

#include "ctx.h"

using namespace xrt;

// what one call asks for, from xrt_denoise_params or xrt_denoise_var_params
struct DenoiseCall {
    DenoiseFilter filter;
    uint32_t width, height, iterations, flags;
    float sigma0;   // Plain: sigma_color; Var: sigma_luminance
    float sigma_normal, sigma_depth, sigma_albedo;
    const float* variance;       // Var: the caller's variance, or null: estimate it over
    uint32_t variance_radius;    // this radius
    float* out_variance;         // Var: null = not wanted
    uint32_t tiled_iterations;   // the first so many iterations may run tiled
};

// a plane of the call: the caller's pointer (null = absent), floats or int32s per pixel, and the
// device pointer the kernels get: the caller's own, or for host memory its place in the staging area
struct DenoisePlane {
    void* user;
    size_t ch;
    void* dev;
};
enum { kColor, kAlbedo, kNormal, kDepth, kObject, kVariance, kOut, kOutVariance, kDenoisePlanes };
static const char* const kPlaneName[kDenoisePlanes] = {"color",  "albedo",   "normal", "depth",
                                                       "object", "variance", "out",    "out_variance"};

// The prepass packs the planes into records; without a caller's variance the variance filter packs
// into col[1] and the estimate writes col[0] = {rgb, estimate} from it.  Then one launch per
// iteration, ping-ponging the colour records; the last writes the outputs.
// d: null when the caller passed no params.  who: the entry point's name in error texts.
// host: color / variance / guides / the outputs are host memory, staged through the context's buffer.
// wait_stream: the device entry point's ordering (xrt_render_aov_device's).
static int denoise_run(xrt_ctx* m, const char* who, const DenoiseCall* d, const float* color, const xrt_aov_buffers* guides,
                       float* out, bool host, hipStream_t wait_stream, xrt_denoise_stats* st) {
    const auto t_start = std::chrono::steady_clock::now();
    const std::string pre = std::string(who) + ": ";
    if (!m || !d || !out) return set_err(m, XRT_ERR_INVALID, pre + "null argument");
    if (d->width == 0 || d->height == 0) return set_err(m, XRT_ERR_INVALID, pre + "bad image size");
    if (d->iterations == 0 || d->iterations > XRT_DENOISE_MAX_ITERATIONS)
        return set_err(m, XRT_ERR_INVALID, pre + "iterations must be 1 .. XRT_DENOISE_MAX_ITERATIONS");
    const bool var = d->filter == DenoiseFilter::Var, estimate = var && !d->variance;
    if (estimate && (d->variance_radius < 1 || d->variance_radius > XRT_DENOISE_VAR_MAX_RADIUS))
        return set_err(m, XRT_ERR_INVALID, pre + "variance_radius must be 1 .. XRT_DENOISE_VAR_MAX_RADIUS without a variance plane");
    xrt_ctx* c = first_device(m);
    auto fail = [&](int rc) { return c == m ? rc : multi_fail(m, c, rc, who); };
    const size_t npix = (size_t)d->width * d->height;
    if (!color && (!c->fb.p || npix * 3 * sizeof(float) > c->fb.bytes))
        return set_err(m, XRT_ERR_STATE, pre + "no framebuffer of that size (render first)");
    int rc = order_after(c, host ? 0 : 2, wait_stream, false);
    if (rc) return set_err(m, rc, c->err);
    const xrt_aov_buffers none{nullptr, nullptr, nullptr, nullptr, nullptr};
    const xrt_aov_buffers& g = guides ? *guides : none;
    DenoisePlane pl[kDenoisePlanes] = {{const_cast<float*>(color), 3, nullptr}, {g.albedo, 3, nullptr}, {g.normal, 3, nullptr},
                                       {g.depth, 1, nullptr}, {g.object, 1, nullptr}, {const_cast<float*>(d->variance), 1, nullptr},
                                       {out, 3, nullptr}, {d->out_variance, 1, nullptr}};
    // records: col[2], nrm, alb; behind them the host entry points' staging, plane after plane
    size_t staged = 0;
    for (const DenoisePlane& q : pl)
        if (host && q.user) staged += q.ch;
    if ((rc = ensure(c, c->denoise, npix * (4 * sizeof(f4) + staged * sizeof(float))))) return fail(rc);
    f4* rec = as<f4>(c->denoise);
    f4 *col[2] = {rec, rec + npix}, *nrm = rec + 2 * npix, *alb = rec + 3 * npix;
    float* s = reinterpret_cast<float*>(rec + 4 * npix);
    for (int k = 0; k < kDenoisePlanes; ++k) {
        DenoisePlane& q = pl[k];
        q.dev = q.user;
        if (!host || !q.user) continue;
        q.dev = s, s += q.ch * npix;
        if (k < kOut && hipMemcpyAsync(q.dev, q.user, npix * q.ch * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return fail(set_err(c, XRT_ERR_HIP, pre + "copy of " + kPlaneName[k]));
    }
    if (!color) pl[kColor].dev = c->fb.p;
    auto plane = [&](int k) { return static_cast<float*>(pl[k].dev); };
    const float sig[3] = {d->sigma_normal, d->sigma_depth, d->sigma_albedo};
    auto inv_sq = [](float sigma) { return sigma > 0.0f ? 1.0f / (sigma * sigma) : 0.0f; };
    xrt_stats S{};
    xrt_denoise_stats D{};
    LaunchTimer T{c, S, (d->flags & XRT_DENOISE_TIMING) != 0, {}, {}};
    hipError_t e = T.launch(XRT_K_STEP, [&] {
        return launch_denoise_pack(plane(kColor), plane(kVariance), plane(kAlbedo), plane(kNormal), plane(kDepth),
                                   static_cast<const int32_t*>(pl[kObject].dev), npix, col[estimate ? 1 : 0], nrm, alb, c->stream);
    });
    if (e != hipSuccess) return fail(hip_err(c, e, "k_dn_pack"));
    if (estimate) {
        e = T.launch(XRT_K_STEP, [&] {
            return launch_dnv_estimate(col[1], nrm, col[0], d->width, d->height, (int)d->variance_radius, c->stream);
        });
        if (e != hipSuccess) return fail(hip_err(c, e, "k_dnv_estimate"));
    }
    for (uint32_t i = 0; i < d->iterations; ++i) {
        const float scale = (float)(1u << (2 * i));
        const bool last = i + 1 == d->iterations;
        const bool tiled = !(d->flags & XRT_DENOISE_NO_TILE) && i < d->tiled_iterations && denoise_has_tiled(1 << i);
        const DenoiseK K{var ? d->sigma0 : inv_sq(d->sigma0) * scale, inv_sq(sig[0]), inv_sq(sig[1]) * (1.0f / scale), inv_sq(sig[2])};
        const DenoiseIter I{col[i & 1], nrm, alb, last ? nullptr : col[(i + 1) & 1], last ? plane(kOut) : nullptr,
                            last ? plane(kOutVariance) : nullptr, d->width, d->height, 1 << i, K};
        e = T.launch(XRT_K_STEP, [&] { return launch_denoise_iter(d->filter, I, tiled, c->stream); });
        if (e != hipSuccess) return fail(hip_err(c, e, tiled ? "k_dn_tiled" : "k_dn_direct"));
        (tiled ? D.tiled_iterations : D.direct_iterations)++;
    }
    for (int k = kOut; k < kDenoisePlanes && e == hipSuccess; ++k)
        if (host && pl[k].user) e = hipMemcpyAsync(pl[k].user, pl[k].dev, npix * pl[k].ch * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(hip_err(c, e, who));
    T.read_out();
    D.kernel_ms = S.kernel_ms[XRT_K_STEP];
    D.launches = (uint32_t)S.launches[XRT_K_STEP];
    D.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (st) *st = D;
    return XRT_OK;
}

static int denoise_plain(xrt_ctx* c, const xrt_denoise_params* p, const float* color, const xrt_aov_buffers* guides, float* out,
                         bool host, hipStream_t wait_stream, xrt_denoise_stats* st) {
    DenoiseCall d{};
    if (p)
        d = DenoiseCall{DenoiseFilter::Plain, p->width, p->height, p->iterations, p->flags, p->sigma_color, p->sigma_normal,
                        p->sigma_depth, p->sigma_albedo, nullptr, 0, nullptr, XRT_DENOISE_TILED_ITERATIONS};
    return denoise_run(c, "xrt_denoise", p ? &d : nullptr, color, guides, out, host, wait_stream, st);
}

static int denoise_var(xrt_ctx* c, const xrt_denoise_var_params* p, const float* color, const float* variance,
                       const xrt_aov_buffers* guides, float* out, float* out_variance, bool host, hipStream_t wait_stream,
                       xrt_denoise_stats* st) {
    DenoiseCall d{};
    if (p)
        d = DenoiseCall{DenoiseFilter::Var, p->width, p->height, p->iterations, p->flags, p->sigma_luminance, p->sigma_normal,
                        p->sigma_depth, p->sigma_albedo, variance, p->variance_radius, out_variance,
                        XRT_DENOISE_VAR_TILED_ITERATIONS};
    return denoise_run(c, "xrt_denoise_var", p ? &d : nullptr, color, guides, out, host, wait_stream, st);
}

extern "C" {

int xrt_denoise(xrt_ctx* c, const xrt_denoise_params* p, const float* color, const xrt_aov_buffers* guides, float* out,
                xrt_denoise_stats* st) {
    return denoise_plain(c, p, color, guides, out, true, nullptr, st);
}

int xrt_denoise_device(xrt_ctx* c, const xrt_denoise_params* p, const float* d_color, const xrt_aov_buffers* d_guides,
                       float* d_out, void* hip_stream, xrt_denoise_stats* st) {
    return denoise_plain(c, p, d_color, d_guides, d_out, false, (hipStream_t)hip_stream, st);
}

int xrt_denoise_var(xrt_ctx* c, const xrt_denoise_var_params* p, const float* color, const float* variance,
                    const xrt_aov_buffers* guides, float* out, float* out_variance, xrt_denoise_stats* st) {
    return denoise_var(c, p, color, variance, guides, out, out_variance, true, nullptr, st);
}

int xrt_denoise_var_device(xrt_ctx* c, const xrt_denoise_var_params* p, const float* d_color, const float* d_variance,
                           const xrt_aov_buffers* d_guides, float* d_out, float* d_out_variance, void* hip_stream,
                           xrt_denoise_stats* st) {
    return denoise_var(c, p, d_color, d_variance, d_guides, d_out, d_out_variance, false, (hipStream_t)hip_stream, st);
}

}  // extern "C"
