// api_query.cpp — the C ABI of include/xrt.h, what runs on a context's first device beside the
// renders: ray queries, the tone map and the device self-tests.
#include "bvh_walk.h"
#include "ctx.h"

using namespace xrt;

extern "C" {

// Scene::intersect / Scene::occluded (Src/scene.cpp:190-211) for caller rays, on the GPU
int xrt_query(xrt_ctx* c, uint32_t n, const float* rays, const float* tmax, int32_t mode, xrt_hit* out) {
    c = first_device(c);
    if (!c || (n && (!rays || !out))) return XRT_ERR_INVALID;
    if (mode != XRT_QUERY_INTERSECT && mode != XRT_QUERY_OCCLUDED) return set_err(c, XRT_ERR_INVALID, "bad query mode");
    if (!c->has_scene) return set_err(c, XRT_ERR_STATE, "upload a scene first");
    if (n == 0) return XRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->ray_o, n * 16)) || (rc = ensure(c, c->ray_d, n * 16)) || (rc = ensure(c, c->hit, n * 16)) ||
        (rc = ensure(c, c->hit2, n * 16)) || (rc = ensure(c, c->hit3, n * 16)) || (rc = ensure(c, c->sh_o, n * 16)) ||
        (rc = ensure(c, c->sh_d, n * 16)) || (rc = ensure(c, c->state, n * 4)) || (rc = ensure(c, c->occ, n * 4)) ||
        (rc = ensure(c, c->lists, (n + 64) * 4)) || (rc = ensure(c, c->counts, 5 * kMaxParts * 4)) ||
        (rc = ensure(c, c->q_rays, (size_t)n * 24)) || (rc = ensure(c, c->q_tmax, (size_t)n * 4)) ||
        (rc = ensure(c, c->q_out, (size_t)n * sizeof(xrt_hit))))
        return rc;
    // (buffers only ever grow, so the render's cap_slots invariant still holds)
    KParams P = c->base;
    P.n_slots = n, P.n_part = 1, P.part_cap = n;
    P.ray_o = as<f4>(c->ray_o), P.ray_d = as<f4>(c->ray_d), P.hit = as<f4>(c->hit), P.hit2 = as<f4>(c->hit2);
    P.hit3 = as<f4>(c->hit3), P.sh_o = as<f4>(c->sh_o), P.sh_d = as<f4>(c->sh_d);
    P.state = as<uint32_t>(c->state), P.occ = as<uint32_t>(c->occ);
    if ((rc = setup_deep(c, P))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->q_rays.p, rays, (size_t)n * 24, hipMemcpyHostToDevice, c->stream));
    if (tmax) HIPCHK(c, hipMemcpyAsync(c->q_tmax.p, tmax, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    uint32_t* cnt = as<uint32_t>(c->counts);
    HIPCHK(c, launch_query(P, as<float>(c->q_rays), tmax ? as<float>(c->q_tmax) : nullptr, mode, as<uint32_t>(c->lists),
                           cnt, cnt + kMaxParts, as<xrt_hit>(c->q_out), c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->q_out.p, (size_t)n * sizeof(xrt_hit), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; ++i) {   // the triangle within its object's mesh
        xrt_hit& q = out[i];
        if (q.primitive >= 0 && q.object >= 0 && (size_t)q.object < c->obj_tri_first.size() &&
            c->obj_tri_first[q.object] >= 0)
            q.primitive -= c->obj_tri_first[q.object];
    }
    return XRT_OK;
}

int xrt_tonemap(xrt_ctx* c, const float* d_rgb, uint32_t n_pixels, float gamma, uint8_t* rgb8_out) {
    c = first_device(c);
    if (!c || !rgb8_out) return XRT_ERR_INVALID;
    const float* src = d_rgb ? d_rgb : as<float>(c->fb);
    if (!src || (!d_rgb && (size_t)n_pixels * 3 * sizeof(float) > c->fb.bytes))
        return set_err(c, XRT_ERR_STATE, "xrt_tonemap: no framebuffer of that size (render first)");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf out;
    int rc;
    const size_t n = (size_t)n_pixels * 3;
    if ((rc = ensure(c, out, n + 16))) return rc;
    hipError_t e = launch_tonemap(src, (uint32_t)n, 1.0f / gamma, as<uint8_t>(out), c->stream);   // Src/image.h:85
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(rgb8_out, out.p, n, hipMemcpyDeviceToHost);
    free_buf(out);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_tonemap");
}

// ---------------------------------------------------------------- self-tests ----
int xrt_test_rng(xrt_ctx* c, const uint32_t* seeds, uint32_t n_seeds, uint32_t skip, uint32_t n, float* out) {
    c = first_device(c);
    if (!c || !seeds || !out) return XRT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf ds, dout, rings;
    int rc;
    if ((rc = ensure(c, ds, n_seeds * 4)) || (rc = ensure(c, dout, (size_t)n_seeds * n * 4)) ||
        (rc = ensure(c, rings, (size_t)n_seeds * kRing * 4)))
        return rc;
    hipError_t e = hipMemcpy(ds.p, seeds, n_seeds * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_test_rng(as<uint32_t>(ds), n_seeds, skip, n, as<float>(dout), as<uint32_t>(rings), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n_seeds * n * 4, hipMemcpyDeviceToHost);
    free_buf(ds), free_buf(dout), free_buf(rings);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_rng");
}

int xrt_test_whitted_math(xrt_ctx* c, const float* in, uint32_t n, float* out) {
    c = first_device(c);
    if (!c || !in || !out) return XRT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf din, dout;
    int rc;
    if ((rc = ensure(c, din, (size_t)n * 24 + 16)) || (rc = ensure(c, dout, (size_t)n * 52 + 16))) {
        free_buf(din), free_buf(dout);
        return rc;
    }
    hipError_t e = hipMemcpy(din.p, in, (size_t)n * 24, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = launch_test_whitted(as<float>(din), n, as<float>(dout), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * 52, hipMemcpyDeviceToHost);
    free_buf(din), free_buf(dout);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_whitted_math");
}

// the camera lists k_camlist builds for the render p describes (spec.hip), 4 words per slot
int xrt_test_camlist(xrt_ctx* c, const xrt_render_params* p, uint32_t* out) {
    c = first_device(c);
    if (!c || !p || !out) return XRT_ERR_INVALID;
    if (!c->has_scene || !c->has_camera) return set_err(c, XRT_ERR_STATE, "upload a scene and set a camera first");
    if (c->base.scene_kind != SCN_TRI || c->base.n_tris < 1 || c->base.n_tris > 64)
        return set_err(c, XRT_ERR_STATE, "xrt_test_camlist: the camera lists are built for a scene of 1 to 64 triangles");
    if (p->width == 0 || p->height == 0 || p->shard_count == 0 || p->shard_index >= p->shard_count)
        return set_err(c, XRT_ERR_INVALID, "bad image size or shard");
    const size_t n = (size_t)shard_rows(p->height, p->shard_index, p->shard_count) * p->width;
    if (n == 0) return XRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->camlist, n * sizeof(uint4)))) return rc;
    KParams P = render_params(c, p, n, nullptr);   // retire = 0: of the slots and the image nothing is touched
    P.camlist = as<uint4>(c->camlist);
    hipError_t e = launch_camlist(P, false, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, c->camlist.p, n * sizeof(uint4), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_camlist");
}

int xrt_test_trig(xrt_ctx* c, const float* x, uint32_t n, float* out) {
    c = first_device(c);
    if (!c || !x || !out) return XRT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf dx, dout;
    int rc;
    if ((rc = ensure(c, dx, (size_t)n * 4 + 16)) || (rc = ensure(c, dout, (size_t)n * 8 + 16))) return rc;
    hipError_t e = hipMemcpy(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_test_trig(as<float>(dx), n, as<float>(dout), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost);
    free_buf(dx), free_buf(dout);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_trig");
}

int xrt_test_logexp(xrt_ctx* c, const float* x, uint32_t n, float* out) {
    c = first_device(c);
    if (!c || !x || !out) return XRT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf dx, dout;
    int rc;
    if ((rc = ensure(c, dx, (size_t)n * 4 + 16)) || (rc = ensure(c, dout, (size_t)n * 8 + 16))) return rc;
    hipError_t e = hipMemcpy(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_test_logexp(as<float>(dx), n, as<float>(dout), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost);
    free_buf(dx), free_buf(dout);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_logexp");
}

int xrt_test_powf(xrt_ctx* c, const float* x, uint32_t n, float y, float* out) {
    c = first_device(c);
    if (!c || !x || !out) return XRT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf dx, dout;
    int rc;
    if ((rc = ensure(c, dx, (size_t)n * 4 + 16)) || (rc = ensure(c, dout, (size_t)n * 4 + 16))) return rc;
    hipError_t e = hipMemcpy(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_test_powf(as<float>(dx), n, y, as<float>(dout), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost);
    free_buf(dx), free_buf(dout);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_powf");
}

int xrt_test_trig_draw_domain(xrt_ctx* c, uint32_t first, uint32_t count, float* out_sin, float* out_cos, float* out_r) {
    c = first_device(c);
    if (!c || !out_sin || !out_cos || !out_r) return XRT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf ds, dc, dr;
    int rc;
    const size_t b = (size_t)count * 4 + 16;
    if ((rc = ensure(c, ds, b)) || (rc = ensure(c, dc, b)) || (rc = ensure(c, dr, b))) return rc;
    hipError_t e = launch_test_trig_domain(first, count, as<float>(ds), as<float>(dc), as<float>(dr), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out_sin, ds.p, (size_t)count * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_cos, dc.p, (size_t)count * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_r, dr.p, (size_t)count * 4, hipMemcpyDeviceToHost);
    free_buf(ds), free_buf(dc), free_buf(dr);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_trig_draw_domain");
}

// the kernels' own medium_density (medium.h) on the context's heterogeneous medium
int xrt_test_density(xrt_ctx* c, const float* points, uint32_t n, float* out, int32_t* layout) {
    c = first_device(c);
    if (!c || !points || !out || !layout) return XRT_ERR_INVALID;
    const DMedium& M = c->base.medium;
    if (!c->has_medium || M.kind != XRT_MEDIUM_HETEROGENEOUS)
        return set_err(c, XRT_ERR_STATE, "xrt_test_density: set a heterogeneous medium first");
    *layout = M.brick_table ? XRT_DENSITY_BRICKS : M.corners ? XRT_DENSITY_CORNERS : XRT_DENSITY_ROWS;
    if (n == 0) return XRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf dp, dout;
    int rc;
    if ((rc = ensure(c, dp, (size_t)n * 12 + 16)) || (rc = ensure(c, dout, (size_t)n * 4 + 16))) {
        free_buf(dp), free_buf(dout);
        return rc;
    }
    hipError_t e = hipMemcpy(dp.p, points, (size_t)n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_test_density(M, as<float>(dp), n, as<float>(dout), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost);
    free_buf(dp), free_buf(dout);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_density");
}

// the kernels' own hg_sample (medium.h), each item's two draws from its own eight raw words
int xrt_test_hg(xrt_ctx* c, float g, const float* wo, const uint32_t* words, uint32_t n, float* wi) {
    c = first_device(c);
    if (!c || !wo || !words || !wi) return XRT_ERR_INVALID;
    if (n == 0) return XRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf dwo, dw, dwi;
    int rc;
    if ((rc = ensure(c, dwo, (size_t)n * 12 + 16)) || (rc = ensure(c, dw, (size_t)n * 32)) ||
        (rc = ensure(c, dwi, (size_t)n * 12 + 16))) {
        free_buf(dwo), free_buf(dw), free_buf(dwi);
        return rc;
    }
    hipError_t e = hipMemcpy(dwo.p, wo, (size_t)n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dw.p, words, (size_t)n * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_test_hg(g, as<float>(dwo), as<uint32_t>(dw), n, as<float>(dwi), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(wi, dwi.p, (size_t)n * 12, hipMemcpyDeviceToHost);
    free_buf(dwo), free_buf(dw), free_buf(dwi);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_hg");
}

// the kernels' own sample_wavelength (medium.h), each item's draw from its own eight raw words
int xrt_test_wavelength(xrt_ctx* c, const float* thr, const float* albedo, const uint32_t* words, uint32_t n,
                        uint32_t* channel, float* pmf) {
    c = first_device(c);
    if (!c || !thr || !albedo || !words || !channel || !pmf) return XRT_ERR_INVALID;
    if (n == 0) return XRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf dt, da, dw, dc, dp;
    int rc;
    if ((rc = ensure(c, dt, (size_t)n * 12 + 16)) || (rc = ensure(c, da, (size_t)n * 12 + 16)) ||
        (rc = ensure(c, dw, (size_t)n * 32)) || (rc = ensure(c, dc, (size_t)n * 4 + 16)) ||
        (rc = ensure(c, dp, (size_t)n * 12 + 16))) {
        free_buf(dt), free_buf(da), free_buf(dw), free_buf(dc), free_buf(dp);
        return rc;
    }
    hipError_t e = hipMemcpy(dt.p, thr, (size_t)n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(da.p, albedo, (size_t)n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dw.p, words, (size_t)n * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = launch_test_wavelength(as<float>(dt), as<float>(da), as<uint32_t>(dw), n, as<uint32_t>(dc), as<float>(dp),
                                   c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(channel, dc.p, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(pmf, dp.p, (size_t)n * 12, hipMemcpyDeviceToHost);
    free_buf(dt), free_buf(da), free_buf(dw), free_buf(dc), free_buf(dp);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_wavelength");
}

// what upload_scene_one built for the walks of the uploaded scene; reads the context only
int xrt_test_bvh_info(xrt_ctx* c, int32_t out[8]) {
    c = first_device(c);
    if (!c || !out) return XRT_ERR_INVALID;
    if (!c->has_scene) return set_err(c, XRT_ERR_STATE, "upload a scene first");
    const KParams& P = c->base;
    const uint32_t entry = P.two_level ? bvh4_lds(P).entry : bvh_lds(P).entry;
    out[0] = P.bvh_nodes, out[1] = P.bvh_stack, out[2] = P.bvh4_nodes, out[3] = P.bvh4_stack;
    out[4] = P.two_level, out[5] = P.n_snode, out[6] = c->bvh_tris;
    out[7] = P.bvh_nodes > 0 ? (int32_t)entry : 0;
    return XRT_OK;
}

}  // extern "C"

// every 32-bit input: mode 0 rcp_rn vs 1/b, mode 1 div_const(x, c, rc) vs x / c (device_math.h)
int xrt_test_fastdiv(xrt_ctx* c, uint32_t mode, float cst, float rc, uint64_t* n_bad, uint32_t* first_bad16) {
    c = first_device(c);
    if (!c || !n_bad || !first_bad16) return XRT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long* d_n = nullptr;
    uint32_t* d_bad = nullptr;
    HIPCHK(c, hipMalloc(&d_n, 8));
    HIPCHK(c, hipMalloc(&d_bad, 64));
    hipError_t e = hipMemsetAsync(d_n, 0, 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0xff, 64, c->stream);
    const uint32_t chunk = 1u << 30;
    for (uint64_t f = 0; f < (1ull << 32) && e == hipSuccess; f += chunk)
        e = launch_test_fastdiv(mode, cst, rc, (uint32_t)f, chunk, d_n, d_bad, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(n_bad, d_n, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(first_bad16, d_bad, 64, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_n);
    (void)hipFree(d_bad);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_fastdiv");
}
