// api_multi.cpp — the C ABI of include/xrt.h, the multi-GPU context.
// ParallelRenderer::render fans the pixel loop out over the whole machine
// (Src/renderer.cpp:83-99); here the machine is the listed GPUs.  Pixels are independent
// (per-pixel seed and accumulation, Src/renderer.cpp:35-36,75), so each of the n devices renders
// every n-th row of the caller's shard (device_shard) — one host thread
// and one HIP stream per device, all devices at once — and the frame is assembled in the
// first device's framebuffer by one strided 2-D copy per other device (its own rows only,
// over xGMI peer access): the same frame a zero-padded sum-reduce would produce, with 1/n
// of the bytes and no arithmetic.  Bit-identical to the one-device render.
#include <chrono>

#include "ctx.h"

namespace xrt {

int multi_fail(xrt_ctx* m, xrt_ctx* s, int rc, const char* what) {
    return set_err(m, rc, std::string(what) + " on device " + std::to_string(s->device) + ": " + s->err);
}

// device i of n's share of the rows p names
static xrt_render_params device_shard(const xrt_render_params* p, uint32_t n, uint32_t i) {
    xrt_render_params q = *p;
    q.shard_count = p->shard_count * n;
    q.shard_index = p->shard_index + p->shard_count * i;
    return q;
}

int fan_out_rows(xrt_ctx* m, const xrt_render_params* p, const char* what,
                 const std::function<int(uint32_t, const xrt_render_params*)>& per_device) {
    const uint32_t n = (uint32_t)m->subs.size();
    std::vector<int> rcs(n, XRT_OK);
    on_threads((int)n, 0, [&](int i) {
        const xrt_render_params q = device_shard(p, n, (uint32_t)i);
        rcs[i] = per_device((uint32_t)i, &q);
    });
    for (uint32_t i = 0; i < n; ++i)
        if (rcs[i] != XRT_OK) return multi_fail(m, m->subs[i], rcs[i], what);
    return XRT_OK;
}

int gather_rows(xrt_ctx* m, const xrt_render_params* p, const std::vector<RowPlane>& planes) {
    xrt_ctx* s0 = m->subs[0];
    const uint32_t n = (uint32_t)m->subs.size();
    HIPCHK(m, hipSetDevice(s0->device));
    for (uint32_t i = 1; i < n; ++i) {
        // device i's rows: y0, then every stride-th
        const xrt_render_params q = device_shard(p, n, i);
        const uint32_t y0 = q.shard_index, stride = q.shard_count, rows = shard_rows(p->height, y0, stride);
        if (rows == 0) continue;
        for (const RowPlane& pl : planes) {
            if (!pl.dev[0]) continue;
            const size_t row = (size_t)p->width * pl.pixel_bytes, pitch = row * stride, off = (size_t)y0 * row;
            HIPCHK(m, hipMemcpy2DAsync(static_cast<char*>(pl.dev[0]) + off, pitch, static_cast<char*>(pl.dev[i]) + off,
                                       pitch, row, rows, hipMemcpyDefault, s0->stream));
        }
    }
    HIPCHK(m, hipStreamSynchronize(s0->stream));
    return XRT_OK;
}

// The only place that combines xrt_stats: a counter added to the structure is added here.
xrt_stats sum_stats(const std::vector<xrt_stats>& S) {
    xrt_stats T = S[0];   // the schedule's description (schedule, partitions, layout) is device 0's
    for (size_t i = 1; i < S.size(); ++i) {
        for (int k = 0; k < XRT_K_COUNT; ++k) T.kernel_ms[k] += S[i].kernel_ms[k], T.launches[k] += S[i].launches[k];
        T.samples += S[i].samples, T.segments += S[i].segments, T.shadow_rays += S[i].shadow_rays;
        T.draws += S[i].draws, T.rejected += S[i].rejected, T.stalled += S[i].stalled;
        T.rng_twists += S[i].rng_twists;
        T.pix_windows += S[i].pix_windows, T.pix_stride4 += S[i].pix_stride4, T.pix_frustum += S[i].pix_frustum;
        T.pix_frustum_overflow += S[i].pix_frustum_overflow, T.pix_shadow_list += S[i].pix_shadow_list;
        T.pix_shadow_overflow += S[i].pix_shadow_overflow, T.pix_flushes += S[i].pix_flushes;
        T.spec_launches += S[i].spec_launches;
        T.whit_rays += S[i].whit_rays, T.whit_depth_cut += S[i].whit_depth_cut;
        T.whit_refract += S[i].whit_refract, T.whit_tir += S[i].whit_tir;
        for (int k = 0; k < 5; ++k) T.layout_launches[k] += S[i].layout_launches[k];
        T.path_slots += S[i].path_slots;
        T.iterations = std::max(T.iterations, S[i].iterations);
    }
    return T;
}

int render_multi(xrt_ctx* m, const xrt_render_params* p, float* d_out, float* h_io, xrt_stats* st, int wait,
                 hipStream_t wait_stream, float* d_var) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!p) return set_err(m, XRT_ERR_INVALID, "null params");
    if (p->width == 0 || p->height == 0 || p->shard_count == 0 || p->shard_index >= p->shard_count)
        return set_err(m, XRT_ERR_INVALID, "bad image size or shard");
    const uint32_t n = (uint32_t)m->subs.size();
    const size_t npix = (size_t)p->width * p->height, bytes = npix * 3 * sizeof(float);
    const bool acc = (p->flags & XRT_FLAG_ACCUMULATE) != 0 && !d_var;   // a variance render refuses it
    xrt_ctx* s0 = m->subs[0];
    int rc = order_after(s0, wait, wait_stream, true);
    if (rc) return set_err(m, rc, s0->err);
    // every device renders into its own framebuffer; device 0 directly into the output
    // ... and a variance render's plane likewise: device 0 into d_var
    std::vector<void*> fbs(n, nullptr), vars(n, nullptr);
    for (uint32_t i = 0; i < n; ++i) {
        xrt_ctx* s = m->subs[i];
        HIPCHK(m, hipSetDevice(s->device));
        if (d_var && i == 0) {
            vars[0] = d_var;
        } else if (d_var) {
            if ((rc = ensure(s, s->var, npix * sizeof(float)))) return multi_fail(m, s, rc, "variance plane");
            vars[i] = s->var.p;
        }
        if (i == 0 && d_out) {
            fbs[0] = d_out;
        } else {
            if ((rc = ensure(s, s->fb, bytes))) return multi_fail(m, s, rc, "framebuffer");
            fbs[i] = s->fb.p;
        }
        if (acc) {   // each device starts its rows from the caller's image
            if (d_out && i > 0)
                HIPCHK(m, hipMemcpy(fbs[i], d_out, bytes, hipMemcpyDefault));
            else if (!d_out)
                HIPCHK(m, hipMemcpy(fbs[i], h_io, bytes, hipMemcpyHostToDevice));
        }
    }
    std::vector<xrt_stats> S(n);
    if ((rc = fan_out_rows(m, p, "render",
                           [&](uint32_t i, const xrt_render_params* q) {
                               return render_impl(m->subs[i], q, static_cast<float*>(fbs[i]), nullptr, &S[i], 0, nullptr,
                                                  static_cast<float*>(vars[i]));
                           })) ||
        (rc = gather_rows(m, p, {RowPlane{fbs, 3 * sizeof(float)}, RowPlane{vars, sizeof(float)}})))
        return rc;
    if (h_io) HIPCHK(m, hipMemcpy(h_io, fbs[0], bytes, hipMemcpyDeviceToHost));
    if (st) {
        *st = sum_stats(S);
        st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return XRT_OK;
}

}  // namespace xrt

using namespace xrt;

extern "C" {

int xrt_create_multi(const int* devices, int n_devices, xrt_ctx** out) {
    if (!out) return XRT_ERR_INVALID;
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) return XRT_ERR_INVALID;
    xrt_ctx* m = new xrt_ctx();
    m->device = devices[0];
    for (int i = 0; i < n_devices; ++i) {
        xrt_ctx* s = nullptr;
        const int rc = xrt_create(devices[i], &s);
        if (rc != XRT_OK) {
            xrt_destroy(m);
            return rc;
        }
        m->subs.push_back(s);
    }
    // peer access from the first device to every other one (for the row gather); devices
    // that cannot map each other fall back to the runtime's staged peer copy
    (void)hipSetDevice(devices[0]);
    for (int i = 1; i < n_devices; ++i) {
        int can = 0;
        if (devices[i] != devices[0] && hipDeviceCanAccessPeer(&can, devices[0], devices[i]) == hipSuccess && can) {
            const hipError_t e = hipDeviceEnablePeerAccess(devices[i], 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
    }
    *out = m;
    return XRT_OK;
}

int xrt_device_count(const xrt_ctx* c) { return !c ? 0 : c->subs.empty() ? 1 : (int)c->subs.size(); }

}  // extern "C"
