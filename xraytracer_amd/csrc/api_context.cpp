// api_context.cpp — the C ABI of include/xrt.h, one device context: create, destroy, errors,
// device buffers and the ordering of a call after the caller's work.
#include "ctx.h"

namespace xrt {

int set_err(xrt_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

int hip_err(xrt_ctx* c, hipError_t e, const char* what) {
    return set_err(c, XRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

void free_buf(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

int ensure(xrt_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return XRT_OK;
    free_buf(b);
    if (bytes == 0) return XRT_OK;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        return set_err(c, XRT_ERR_OOM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    }
    b.bytes = bytes;
    return XRT_OK;
}

int upload(xrt_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    int rc = ensure(c, b, std::max<size_t>(bytes, 16));
    if (rc) return rc;
    if (bytes) HIPCHK(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return XRT_OK;
}

int order_after(xrt_ctx* c, int wait, hipStream_t wait_stream, bool host_blocks) {
    HIPCHK(c, hipSetDevice(c->device));
    if (wait == 1) {
        HIPCHK(c, hipDeviceSynchronize());
    } else if (wait == 2) {
        HIPCHK(c, hipEventRecord(c->wait_ev, wait_stream));
        if (host_blocks)
            HIPCHK(c, hipEventSynchronize(c->wait_ev));
        else
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->wait_ev, 0));
    }
    return XRT_OK;
}

}  // namespace xrt

using namespace xrt;

extern "C" {

int xrt_abi_version(void) { return XRT_ABI_VERSION; }

int xrt_create(int device, xrt_ctx** out) {
    if (!out) return XRT_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return XRT_ERR_HIP;
    if (device < 0 || device >= n) return XRT_ERR_INVALID;
    xrt_ctx* c = new xrt_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void**)&c->h_poll, 8 * kMaxStepGroups * kMaxParts * sizeof(uint32_t), hipHostMallocDefault) !=
            hipSuccess ||
        hipEventCreateWithFlags(&c->wait_ev, hipEventDisableTiming) != hipSuccess) {
        xrt_destroy(c);
        return XRT_ERR_HIP;
    }
    for (auto& slot : c->poll_ev)
        for (hipEvent_t& e : slot)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                xrt_destroy(c);
                return XRT_ERR_HIP;
            }
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || lds <= 0) {
        xrt_destroy(c);
        return XRT_ERR_HIP;
    }
    c->base.lds_max = (uint32_t)lds;
    *out = c;
    return XRT_OK;
}

void xrt_destroy(xrt_ctx* c) {
    if (!c) return;
    for (xrt_ctx* s : c->subs) xrt_destroy(s);
    c->subs.clear();
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipStream_t s : c->group_stream)   // joined into c->stream after every render; synchronised all the same
        if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    for (hipEvent_t e : c->join_ev)
        if (e) (void)hipEventDestroy(e);
    DevBuf* all[] = {&c->tri, &c->tri_ng, &c->tri_nrm, &c->sph, &c->sph_obj, &c->box, &c->objs, &c->lights,
                     &c->segs, &c->density, &c->obj_box, &c->obj_plane, &c->bvh_node, &c->bvh_tri, &c->snode, &c->ssph, &c->sbk, &c->sblk, &c->ray_o, &c->ray_d, &c->thr, &c->rad, &c->thr_prev, &c->hit,
                     &c->hit2, &c->hit3, &c->sh_o, &c->sh_d, &c->sh_c, &c->med, &c->med2, &c->nee, &c->state,
                     &c->sample_k, &c->depth, &c->occ, &c->rng_c, &c->rng_g, &c->ring, &c->c_seg, &c->c_shadow,
                     &c->c_rej, &c->c_stall, &c->lists, &c->counts, &c->stats, &c->fb, &c->scratch, &c->kparams};
    for (DevBuf* b : all) free_buf(*b);
    free_buf(c->stri), free_buf(c->sbox), free_buf(c->splane), free_buf(c->bvh4), free_buf(c->deep);
    free_buf(c->q_rays), free_buf(c->q_tmax), free_buf(c->q_out);
    free_buf(c->brick_table), free_buf(c->brick_data), free_buf(c->corners), free_buf(c->camlist);
    free_buf(c->dlights), free_buf(c->obj_albedo), free_buf(c->aov), free_buf(c->denoise);
    free_buf(c->mom), free_buf(c->var), free_buf(c->chunks);
    free_buf(c->acc);
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    for (auto& slot : c->poll_ev)
        for (hipEvent_t e : slot)
            if (e) (void)hipEventDestroy(e);
    if (c->wait_ev) (void)hipEventDestroy(c->wait_ev);
    if (c->h_poll) (void)hipHostFree(c->h_poll);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* xrt_last_error(const xrt_ctx* c) { return c ? c->err.c_str() : "no context (xrt_create failed: no HIP device?)"; }

}  // extern "C"
