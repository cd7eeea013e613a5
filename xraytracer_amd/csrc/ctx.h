// ctx.h — the device context behind xrt_ctx, and what the translation units of the C ABI
// (api_*.cpp) need from each other.  Nothing here is exported: hidden visibility.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "launch.h"
#include "wavefront.h"
#include "xrt.h"

#pragma GCC visibility push(hidden)

namespace xrt {
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// An open progressive session (xrt_progressive_*, api_progressive.cpp).  Between its passes the slots'
// streams (ring, rng_c, rng_g), their counters (c_*) and moments records (mom) and the accumulator are
// the session's state: whatever seeds the slots anew or changes what they render ends it
// (end_progressive).
struct ProgressiveSession {
    bool active = false;
    xrt_render_params p{};     // as given to begin, with the session's schedule flags (spp: unused)
    bool variance = false;     // XRT_PROGRESSIVE_VARIANCE
    size_t n = 0;              // the shard's slots
    uint32_t spp_done = 0, passes = 0, resume_twists = 0;
    uint64_t twists = 0;       // ring twists of the slots so far (xrt_stats::rng_twists is per add)
};

}  // namespace xrt

struct xrt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // scene
    xrt::DevBuf tri, tri_ng, tri_nrm, sph, sph_obj, box, objs, lights, segs, density, obj_box, obj_plane, bvh_node,
        bvh_tri, snode, ssph, sbk, sblk, stri, sbox, splane, bvh4;
    xrt::KParams base{};
    xrt::StepObjs step_objs{};   // kernel-argument object records of the merged-trace schedule
    xrt::StepObjs sstep{};       // two-level trace: the small objects' records (KParams::sstep)
    bool has_scene = false, has_camera = false, has_medium = false;
    int bvh_tris = 0;            // triangles in the triangle BVH's reordered array (xrt_test_bvh_info)
    // WhittedIntegrator: the delta lights (kept across scene uploads), and whether the scene
    // holds a metal / glass object (valid only under Whitted) or a glass one (depth limit)
    xrt::DevBuf dlights;
    bool has_mirror = false, has_glass = false;
    // slots
    size_t cap_slots = 0;
    xrt::DevBuf ray_o, ray_d, thr, rad, thr_prev, hit, hit2, hit3, sh_o, sh_d, sh_c, med, med2, nee;
    xrt::DevBuf state, sample_k, depth, occ, rng_c, rng_g, ring, c_seg, c_shadow, c_rej, c_stall, lists, deep, camlist;
    xrt::DevBuf counts, stats, fb, scratch, kparams;
    // xrt_render_var: per slot the {s1, s2} luminance moments (float2), and the context's own
    // variance plane (host output, sub-contexts of a multi render)
    xrt::DevBuf mom, var;
    xrt::DevBuf chunks;   // the merged schedule's chunk phase: header, counters and list segments (step_chunks.h)
    uint32_t* h_poll = nullptr;  // pinned: LivePoll's 8 slots of kMaxParts counts for each of kMaxStepGroups groups
    std::vector<hipEvent_t> events;   // LaunchTimer's pairs
    hipEvent_t poll_ev[8][xrt::kMaxStepGroups] = {};  // LivePoll's events (created once), slot by group
    hipEvent_t wait_ev = nullptr;   // xrt_render_device_after: the caller stream's position
    // the merged schedule's partition groups (step_groups.h): a stream per group, created with
    // the first render that runs grouped (group_streams), and the events by which they leave
    // the context's stream and come back to it
    hipStream_t group_stream[xrt::kMaxStepGroups] = {};
    hipEvent_t fork_ev = nullptr, join_ev[xrt::kMaxStepGroups] = {};
    // multi-GPU context (xrt_create_multi): one sub-context per device, each rendering an
    // interleaved row shard; the frame is assembled in subs[0]'s framebuffer
    std::vector<xrt_ctx*> subs;
    // ray queries (xrt_query): per object, its first triangle in the device arrays (-1: not
    // a mesh), and the query's own buffers
    std::vector<int> obj_tri_first;
    xrt::DevBuf q_rays, q_tmax, q_out;
    xrt::DevBuf brick_table, brick_data;   // sparse medium (xrt_set_medium_bricks)
    xrt::DevBuf corners;                   // dense medium: per-cell corner values (DMedium::corners)
    // the most bytes the corner values may take; a larger grid reads its rows (xrt_test_corner_grid_limit)
    size_t corner_limit = size_t(2) << 30;
    // guide buffers (xrt_render_aov): per object the albedo as uploaded (3 floats; DObj keeps
    // only albedo / PI), and the context's own planes (host output, sub-contexts of a multi render)
    xrt::DevBuf obj_albedo, aov;
    // xrt_denoise, xrt_denoise_var: the per-pixel records (two colour buffers, normal, albedo: 16 B
    // each), then for the host entry points the staged input planes and the output planes
    xrt::DevBuf denoise;
    // xrt_progressive_*: the open session and its accumulator [H][W][3], the pixels' undivided sums
    xrt::ProgressiveSession prog;
    xrt::DevBuf acc;
};

namespace xrt {

// ---- api_context.cpp: errors and device buffers
int set_err(xrt_ctx* c, int code, const std::string& msg);
int hip_err(xrt_ctx* c, hipError_t e, const char* what);

#define HIPCHK(ctx, expr)                                    \
    do {                                                     \
        hipError_t e_ = (expr);                              \
        if (e_ != hipSuccess) return hip_err(ctx, e_, #expr); \
    } while (0)

void free_buf(DevBuf& b);
int ensure(xrt_ctx* c, DevBuf& b, size_t bytes);   // buffers only grow
int upload(xrt_ctx* c, DevBuf& b, const void* src, size_t bytes);

template <typename T>
T* as(DevBuf& b) {
    return reinterpret_cast<T*>(b.p);
}

// rows y % n == idx of an image of h rows
inline uint32_t shard_rows(uint32_t h, uint32_t idx, uint32_t n) { return idx < h ? (h - idx + n - 1) / n : 0; }

// fn(0) .. fn(n - 1) at once: the first `own` of them on the calling thread, one after the
// other, each of the rest on a thread of its own; returns when all have
template <typename F>
void on_threads(int n, int own, F&& fn) {
    std::vector<std::thread> th;
    for (int t = own; t < n; ++t) th.emplace_back([&fn, t] { fn(t); });
    for (int t = 0; t < own; ++t) fn(t);
    for (auto& t : th) t.join();
}

// What a call must come after, and c's device made current.  wait: 0 = nothing, 1 = the whole
// device, 2 = the work queued on the caller's stream `wait_stream`, for which c's stream
// waits — or, with host_blocks, the host (a multi context's devices start from host threads)
int order_after(xrt_ctx* c, int wait, hipStream_t wait_stream, bool host_blocks);

// ---- api_render.cpp
// Counts every launch into xrt_stats::launches and, with XRT_FLAG_TIMING, puts a pair of the
// context's events round it; read_out, once the stream is synchronised, turns the pairs into
// kernel_ms (and the per-launch trace of experiment builds).
struct LaunchTimer {
    xrt_ctx* c;
    xrt_stats& S;
    bool timing;
    std::vector<int> kids;             // launch q: kernel id (its events: 2q, 2q + 1)
    std::vector<uint64_t> step_live;   // fused loop: the live hint each step launch was sized with

    template <typename F>
    hipError_t launch(int kid, F&& fn) {
        const size_t e = 2 * kids.size();
        bool timed = timing;
        while (timed && c->events.size() < e + 2) {   // created on first use, kept by the context
            hipEvent_t ev;
            if ((timed = hipEventCreate(&ev) == hipSuccess)) c->events.push_back(ev);
        }
        if (timed) kids.push_back(kid);
        if (timed) (void)hipEventRecord(c->events[e], c->stream);
        const hipError_t err = fn();
        if (timed) (void)hipEventRecord(c->events[e + 1], c->stream);
        S.launches[kid]++;
        return err;
    }
    // Launches that overlap on other streams, timed as one span with one pair: span_begin on
    // c->stream before they fork off it, span_end once they have joined it again.  The caller
    // counts the launches.
    bool span_open = false;
    size_t span_stop = 0;   // the open span's second event
    void span_begin(int kid) {
        const size_t e = 2 * kids.size();
        bool timed = timing;
        while (timed && c->events.size() < e + 2) {
            hipEvent_t ev;
            if ((timed = hipEventCreate(&ev) == hipSuccess)) c->events.push_back(ev);
        }
        if (!timed) return;
        kids.push_back(kid);
        (void)hipEventRecord(c->events[e], c->stream);
        span_open = true, span_stop = e + 1;
    }
    void span_end() {
        if (span_open) (void)hipEventRecord(c->events[span_stop], c->stream);
        span_open = false;
    }
    void read_out();
};

// A render's live lists: two slot lists of n_part * part_cap entries that the launches
// ping-pong between (KParams::req, the refill request list, lies behind them), and counter
// arrays of kMaxParts words: three live counters that the loops rotate, then two request
// counters.  k_seed asks for every slot's first ring twist in req(0); the seeding refill
// consumes it and clears req(1), which every later launch is handed (they twist in-line).
struct LiveLists {
    uint32_t* list[2];
    uint32_t* cbase;
    uint32_t* counts(uint64_t j) const { return cbase + (size_t)j * kMaxParts; }
    uint32_t* req(int j) const { return counts(3 + j); }
};

int setup_deep(xrt_ctx* c, KParams& P);   // the two-level trace queues (KParams::deep)
int grow_slots(xrt_ctx* c, size_t n);
KParams render_params(xrt_ctx* c, const xrt_render_params* p, size_t n, float* fb);

// The pieces of render_impl's sequence, which a progressive session runs in an order of its own
// (api_progressive.cpp: seeding in begin; resume, run and finish in every add).
int check_render(xrt_ctx* c, const xrt_render_params* p);   // what every render entry point refuses
// The schedule of one render, decided once (plan_render) before anything is launched: the
// loops, the launchers' arguments and xrt_stats all read it from here.
struct RenderPlan {
    int schedule;       // XRT_SCHED_*
    bool volumetric;    // VPT / VPT-NEE: unbounded walks
    // pixel: one k_pixel launch between k_seed and k_finish, no live lists, no refill, no
    // loop (fused and merged are then only what sized the partitions).  Otherwise fused: the
    // k_step loop (else k_shade + k_trace); merged: its k_step_merged form; two_level: that
    // kernel with the wave's own BVH walk; step_tri: k_step_tri in place of k_step; spec:
    // k_step_spec in the merged schedule's group layouts, which needs the camera lists.
    // whitted: WhittedIntegrator — pixel's shape (one launch, no lists), k_whitted in it, or
    // (whitted_bvh) k_whitted_bvh for a scene beyond LDS under XRT_FLAG_WHITTED_BVH
    // elide: GI in the merged schedule over at most 64 triangles — k_camlist runs right after the
    // seeding refill, with or without speculative launches, and finishes the pixels no camera
    // ray can hit (spec.hip)
    bool pixel, fused, merged, two_level, step_tri, spec, camlist, elide, whitted, whitted_bvh;
    uint32_t n_part, part_cap;                     // live-list partitions
    uint32_t groups;                               // partition groups of the merged schedule's full-wave launches (1: none)
    uint32_t slot_mul;                             // the slot -> pixel map (slot_map.h): 0 row-major, else interleaved
    uint32_t step_visits, spec_visits, rng_keep;   // segments per slot per launch; ring words a launch may need
    uint64_t poll_every, ahead;                    // LivePoll cadence
    uint64_t cap_iters;                            // loop iterations at most
    // the whole-wave phase in block-owned chunks (step_chunks.h): passes per block per launch (0: the
    // grouped schedule from the first round on) and the chunks per class its buffers hold
    uint32_t chunk_passes, chunk_class_cap;
    bool chunk_forced;   // by XRT_FLAG_CHUNKS: the phase runs however many chunks the build leaves (build_chunks)
    // a variance render (xrt_render_var): the slots' {s1, s2} records, which select the moments
    // builds of k_shade / k_whitted / k_whitted_bvh and, under XRT_FLAG_VAR_FUSED, of k_step /
    // k_step_tri / k_step_merged; null for a plain render
    float2* mom;
};
RenderPlan plan_render(const KParams& P, const xrt_render_params* p, float2* mom);
int bind_plan(xrt_ctx* c, KParams& P, const RenderPlan& R, LiveLists& L);
int seed_paths(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, LaunchTimer& T);
int build_chunks(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, LaunchTimer& T, ChunkBufs& B);
int run_paths(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, const ChunkBufs& CB, LaunchTimer& T,
              uint64_t& it, bool& done);
int check_drained(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, uint64_t it);
int read_stats(xrt_ctx* c, const KParams& P, xrt_stats& S);
void plan_stats(const KParams& P, const RenderPlan& R, uint64_t it, xrt_stats& S);
// what seeds the slots anew, or changes the scene, camera, medium or lights they render, ends the session
inline void end_progressive(xrt_ctx* c) {
    if (c) c->prog.active = false;
}
// wait, wait_stream: order_after's.  d_var: a variance render (xrt_render_var) — the device plane
// [height][width] that gets the variance of each pixel's mean luminance; null: a plain render
// probe: xrt_test_chunk_plan — the plan's chunk phase and, when it has one, the chunks built after
// seeding; the call then returns without rendering
struct ChunkProbe {
    uint32_t passes, chunks, blocks, cap;   // passes per launch (0: no phase); chunks that hold a slot; blocks of a launch; chunks the buffers hold
    uint32_t* sizes;                        // live slots of chunk q < min(cap, n_sizes)
    uint32_t n_sizes;
};
int render_impl(xrt_ctx* c, const xrt_render_params* p, float* d_out, float* h_out, xrt_stats* st, int wait = 0,
                hipStream_t wait_stream = nullptr, float* d_var = nullptr, ChunkProbe* probe = nullptr);

// ---- api_multi.cpp: the multi-GPU context
// its first device, where frames and planes are assembled (a single-device context: itself)
inline xrt_ctx* first_device(xrt_ctx* c) { return c && !c->subs.empty() ? c->subs[0] : c; }

int multi_fail(xrt_ctx* m, xrt_ctx* s, int rc, const char* what);

// one(device) for every device of c — for c itself when it is a single device, or null
template <typename F>
int for_each_device(xrt_ctx* c, const char* what, F&& one) {
    if (!c || c->subs.empty()) return one(c);
    for (xrt_ctx* d : c->subs) {
        const int rc = one(d);
        if (rc) return multi_fail(c, d, rc, what);
    }
    return XRT_OK;
}

// per_device(i, q) for every device i of m at once, q the device's share of the shard p
// names; the first failure as multi_fail(.., what)
int fan_out_rows(xrt_ctx* m, const xrt_render_params* p, const char* what,
                 const std::function<int(uint32_t, const xrt_render_params*)>& per_device);

// a plane of the image on every device: dev[0] is where it is assembled (null: plane not
// wanted), dev[i] holds device i's rows
struct RowPlane {
    std::vector<void*> dev;
    size_t pixel_bytes;
};
// the rows fan_out_rows gave the other devices into device 0's planes; complete on return
int gather_rows(xrt_ctx* m, const xrt_render_params* p, const std::vector<RowPlane>& planes);

xrt_stats sum_stats(const std::vector<xrt_stats>& S);   // the devices' stats as one (wall_ms: device 0's)

// d_out: the caller's device image on subs[0]'s GPU (or null: host image h_io); d_var: render_impl's,
// on subs[0]'s GPU
int render_multi(xrt_ctx* m, const xrt_render_params* p, float* d_out, float* h_io, xrt_stats* st, int wait,
                 hipStream_t wait_stream, float* d_var = nullptr);

}  // namespace xrt

#pragma GCC visibility pop
