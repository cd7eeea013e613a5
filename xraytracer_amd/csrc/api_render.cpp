// api_render.cpp — the C ABI of include/xrt.h, one device's render: the wavefront pass schedule
// that replaces NormalRenderer::render / ParallelRenderer::render (Src/renderer.cpp:8-27, 83-99).
// render_impl below is the sequence; each step is one of the pieces before it.
#include <sched.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "ctx.h"

namespace xrt {

// two-level trace queues (KParams::deep): per partition part_cap extension-ray entries, then
// the shadow rays from entry part_cap on — part_cap per light of the trace kernel, which is
// instantiated for at least one light (an occluded query on a light-less scene queues its
// rays as shadow rays of light 0) — then kMaxParts counts, fetch counters and shadow counts
int setup_deep(xrt_ctx* c, KParams& P) {
    P.deep = nullptr, P.deep_count = nullptr, P.deep_cap = 0;
    if (!P.two_level) return XRT_OK;
    P.deep_cap = P.part_cap * (1u + (uint32_t)std::max(1, P.n_lights));
    const size_t words = (size_t)P.n_part * P.deep_cap + 3 * kMaxParts;   // queues, counts, fetch counters
    const int rc = ensure(c, c->deep, words * 4);
    if (rc) return rc;
    P.deep = as<uint32_t>(c->deep);
    P.deep_count = P.deep + (size_t)P.n_part * P.deep_cap;
    return XRT_OK;
}

namespace {

// Is the device's div_const(x, c, RN(1/c)) — q = x * rc, q + (x - c q) * rc with two fmas —
// equal to the IEEE quotient x / c for every x it is used on?  Within div_const's window
// (x exponent 25..248) the computation scales exactly with x's exponent (a residual small
// enough to be subnormal is far below ulp(q) / 2 and cannot change the result), so one
// binade decides it: all 2^23 mantissas of x in [1, 2) are compared with the host's IEEE
// division (SSE, correctly rounded).  c is limited to [2^-4, 2^20] so the window's quotients
// stay normal.  About 10 ms per divisor on 8 threads.  Results are cached process-wide
// (all contexts, including the sub-contexts of xrt_create_multi, share one table under a
// mutex, so a multi-GPU render proves each divisor once), and the check uses at most as many
// threads as the process's CPU affinity mask allows (capped at 8).
bool cdiv_exact(xrt_ctx*, float d) {
    if (!(d >= 0x1p-4f && d <= 0x1p20f)) return false;
    uint32_t key;
    std::memcpy(&key, &d, 4);
    static std::mutex mu;
    static std::unordered_map<uint32_t, bool> cache;
    std::lock_guard<std::mutex> lock(mu);   // held during the check: concurrent callers wait for it
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    const float rc = 1.0f / d;
    int nthreads = 1;
    {
        cpu_set_t cs;
        CPU_ZERO(&cs);
        if (sched_getaffinity(0, sizeof(cs), &cs) == 0) nthreads = CPU_COUNT(&cs);
        nthreads = std::max(1, std::min(nthreads, 8));
    }
    std::vector<char> part(nthreads, 1);
    on_threads(nthreads, 1, [&](int t) {
        bool ok = true;
        for (uint32_t m = (uint32_t)t; m < (1u << 23) && ok; m += (uint32_t)nthreads) {
            const uint32_t xb = 0x3f800000u | m;
            float x;
            std::memcpy(&x, &xb, 4);
            const float q = x * rc;
            ok = std::fma(std::fma(-d, q, x), rc, q) == x / d;
        }
        part[t] = ok;
    });
    bool ok = true;
    for (char p : part) ok &= p != 0;
    cache[key] = ok;
    return ok;
}

}  // namespace

int check_render(xrt_ctx* c, const xrt_render_params* p) {
    if (!c || !p) return XRT_ERR_INVALID;
    if (!c->has_scene || !c->has_camera) return set_err(c, XRT_ERR_STATE, "upload a scene and set a camera first");
    if (p->width == 0 || p->height == 0 || p->shard_count == 0 || p->shard_index >= p->shard_count)
        return set_err(c, XRT_ERR_INVALID, "bad image size or shard");
    if (p->integrator < XRT_INTEGRATOR_GI || p->integrator > XRT_INTEGRATOR_WHITTED)
        return set_err(c, XRT_ERR_INVALID, "unknown integrator");
    if (p->integrator != XRT_INTEGRATOR_WHITTED && c->has_mirror)
        return set_err(c, XRT_ERR_UNSUPPORTED,
                       "the scene holds a metal or glass object: only WhittedIntegrator knows those materials");
    if (p->integrator == XRT_INTEGRATOR_WHITTED && c->has_glass && p->max_depth > XRT_WHITTED_MAX_DEPTH)
        return set_err(c, XRT_ERR_UNSUPPORTED, "WhittedIntegrator over a scene with glass: max_depth above " +
                                                   std::to_string(XRT_WHITTED_MAX_DEPTH) + " (XRT_WHITTED_MAX_DEPTH)");
    const bool volumetric = p->integrator == XRT_INTEGRATOR_VPT || p->integrator == XRT_INTEGRATOR_VPT_NEE;
    if (volumetric && !c->has_medium)
        return set_err(c, XRT_ERR_STATE, "VolumePathTracing needs xrt_set_medium first");
    if (p->integrator == XRT_INTEGRATOR_VPT_NEE && c->base.n_lights == 0)
        return set_err(c, XRT_ERR_STATE, "VolumePathTracingNEE needs an area light");
    if (p->slots_per_wave != 0 && p->slots_per_wave != 4 && p->slots_per_wave != 8 && p->slots_per_wave != 16 &&
        p->slots_per_wave != 32 && p->slots_per_wave != 64)
        return set_err(c, XRT_ERR_INVALID, "slots_per_wave must be 0, 4, 8, 16, 32 or 64");
    if (p->visits_per_launch > 128) return set_err(c, XRT_ERR_INVALID, "visits_per_launch must be 0..128");
    return XRT_OK;
}

namespace {

// what a variance render refuses beyond check_render
int check_render_var(xrt_ctx* c, const xrt_render_params* p) {
    if (p->spp < 2) return set_err(c, XRT_ERR_INVALID, "xrt_render_var: spp must be at least 2 (one sample has no variance)");
    if (p->flags & XRT_FLAG_ACCUMULATE)
        return set_err(c, XRT_ERR_UNSUPPORTED,
                       "xrt_render_var: XRT_FLAG_ACCUMULATE (the moments of the earlier calls' samples are unknown)");
    return XRT_OK;
}

// a shard that owns no rows (shard_index >= height): an all-zero framebuffer
int render_empty_shard(xrt_ctx* c, const xrt_render_params* p, float* d_out, float* h_out, float* d_var, xrt_stats* st,
                       std::chrono::steady_clock::time_point t_start) {
    const size_t npix = (size_t)p->width * p->height;
    int rc;
    if (!d_out && (rc = ensure(c, c->fb, npix * 3 * sizeof(float)))) return rc;
    float* fb0 = d_out ? d_out : as<float>(c->fb);
    if (p->flags & XRT_FLAG_ACCUMULATE) return XRT_OK;   // nothing owned, nothing touched
    HIPCHK(c, hipMemsetAsync(fb0, 0, npix * 3 * sizeof(float), c->stream));
    if (d_var) HIPCHK(c, hipMemsetAsync(d_var, 0, npix * sizeof(float), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_out) HIPCHK(c, hipMemcpy(h_out, fb0, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (st) {
        std::memset(st, 0, sizeof(*st));
        st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return XRT_OK;
}

void bind_slots(xrt_ctx* c, KParams& P) {
    P.ray_o = as<f4>(c->ray_o), P.ray_d = as<f4>(c->ray_d), P.thr = as<f4>(c->thr), P.rad = as<f4>(c->rad);
    P.thr_prev = as<f4>(c->thr_prev), P.hit = as<f4>(c->hit), P.hit2 = as<f4>(c->hit2), P.hit3 = as<f4>(c->hit3);
    P.sh_o = as<f4>(c->sh_o), P.sh_d = as<f4>(c->sh_d), P.sh_c = as<f4>(c->sh_c);
    P.med = as<f4>(c->med), P.med2 = as<f4>(c->med2), P.nee = as<f4>(c->nee);
    P.state = as<uint32_t>(c->state), P.sample_k = as<uint32_t>(c->sample_k), P.depth = as<uint32_t>(c->depth);
    P.occ = as<uint32_t>(c->occ), P.rng_c = as<uint32_t>(c->rng_c), P.rng_g = as<uint32_t>(c->rng_g);
    P.ring = as<uint32_t>(c->ring);
    P.c_seg = as<uint32_t>(c->c_seg), P.c_shadow = as<uint32_t>(c->c_shadow), P.c_rej = as<uint32_t>(c->c_rej);
    P.c_stall = as<uint32_t>(c->c_stall);
    P.stats = as<unsigned long long>(c->stats);
}

}  // namespace

// per-slot path state for n slots (buffers only grow), the live-list counters, the stats
// words and the device copy of KParams
int grow_slots(xrt_ctx* c, size_t n) {
    int rc;
    if (n > c->cap_slots) {
        const size_t L = kMaxLights;
        if ((rc = ensure(c, c->ray_o, n * 16)) || (rc = ensure(c, c->ray_d, n * 16)) || (rc = ensure(c, c->thr, n * 16)) ||
            (rc = ensure(c, c->rad, n * 16)) || (rc = ensure(c, c->thr_prev, n * 16)) || (rc = ensure(c, c->hit, n * 16)) ||
            (rc = ensure(c, c->hit2, n * 16)) || (rc = ensure(c, c->hit3, n * 16)) ||
            (rc = ensure(c, c->sh_o, L * n * 16)) || (rc = ensure(c, c->sh_d, L * n * 16)) ||
            (rc = ensure(c, c->sh_c, L * n * 16)) || (rc = ensure(c, c->med, n * 16)) || (rc = ensure(c, c->med2, n * 16)) ||
            (rc = ensure(c, c->nee, 4 * n * 16)) ||
            (rc = ensure(c, c->state, n * 4)) || (rc = ensure(c, c->sample_k, n * 4)) || (rc = ensure(c, c->depth, n * 4)) ||
            (rc = ensure(c, c->occ, n * 4)) || (rc = ensure(c, c->rng_c, n * 4)) || (rc = ensure(c, c->rng_g, n * 4)) ||
            (rc = ensure(c, c->ring, n * kRing * 4)) || (rc = ensure(c, c->c_seg, n * 4)) ||
            (rc = ensure(c, c->c_shadow, n * 4)) || (rc = ensure(c, c->c_rej, n * 4)) || (rc = ensure(c, c->c_stall, n * 4)) ||
            (rc = ensure(c, c->lists, 3 * (n + kMaxParts) * 4)))   // two live lists + the refill list
            return rc;
        c->cap_slots = n;
    }
    if ((rc = ensure(c, c->counts, 5 * kMaxParts * 4)) || (rc = ensure(c, c->stats, 512))) return rc;
    return ensure(c, c->kparams, sizeof(KParams));
}

// the scene's parameters with this render's image, shard and flags; the schedule's share
// (partitions, rng_keep, queues, lists) follows from plan_render
KParams render_params(xrt_ctx* c, const xrt_render_params* p, size_t n, float* fb) {
    KParams P = c->base;
    P.integrator = p->integrator;
    P.max_depth = p->max_depth, P.width = p->width, P.height = p->height, P.spp = p->spp;
    P.fw = (float)p->width, P.fh = (float)p->height, P.rw = 1.0f / P.fw, P.rh = 1.0f / P.fh;
    P.raspect = 1.0f / P.aspect;
    P.cdiv = (cdiv_exact(c, P.fw) ? 1u : 0u) | (cdiv_exact(c, P.fh) ? 2u : 0u) | (cdiv_exact(c, P.aspect) ? 4u : 0u);
    P.shard_index = p->shard_index, P.shard_count = p->shard_count, P.n_slots = (uint32_t)n;
    P.spw_req = p->slots_per_wave, P.rflags = p->flags & ~kRflagSession;   // the bit is a session's to set (progressive_add)
    // two-level traces: the BVH walk takes four lanes per queued ray (k_trace_deep4q, every
    // size: its lanes keep their own best hits) unless the caller asks for one
    const char* dq = exp_env("XRT_DEEP_QUAD");
    P.deep_quad = dq ? std::atoi(dq) : (p->flags & XRT_FLAG_DEEP_SINGLE) ? 0 : 1;
    bind_slots(c, P);
    P.fb = fb;
    P.camlist = nullptr;
    P.slot_mul = 0;   // the row-major map, unless the render's plan interleaves (plan_render)
    return P;
}

void LaunchTimer::read_out() {
    if (!timing) return;
    const bool trace = exp_env("XRT_TRACE_LAUNCHES") != nullptr;   // experiments: per-launch times
    size_t step_idx = 0;
    for (size_t q = 0; q < kids.size(); ++q) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->events[2 * q], c->events[2 * q + 1]) == hipSuccess) S.kernel_ms[kids[q]] += ms;
        if (trace) {
            float gap = 0.0f;
            if (q) (void)hipEventElapsedTime(&gap, c->events[2 * q - 1], c->events[2 * q]);
            std::fprintf(stderr, "[xrt] launch %zu kernel %d %.3f ms (gap %.3f)%s", q, kids[q], ms, gap,
                         kids[q] == XRT_K_STEP && q < step_live.size() + 2 ? "" : "\n");
            if (kids[q] == XRT_K_STEP) {
                const size_t si = step_idx++;
                std::fprintf(stderr, " live %llu\n", si < step_live.size() ? (unsigned long long)step_live[si] : 0ull);
            }
        }
    }
}

static_assert(XRT_STEP_GROUPS >= 1 && XRT_STEP_GROUPS <= (int)kMaxStepGroups, "XRT_STEP_GROUPS: 1..3");

// The schedule of one render (RenderPlan, ctx.h), decided once before anything is launched
RenderPlan plan_render(const KParams& P, const xrt_render_params* p, float2* mom) {
    RenderPlan R{};
    R.mom = mom;
    const size_t n = P.n_slots;
    R.volumetric = p->integrator == XRT_INTEGRATOR_VPT || p->integrator == XRT_INTEGRATOR_VPT_NEE;
    // The fused k_step (scene resident in LDS, step_visits path segments per slot per launch,
    // in-kernel compaction and ring refills) when the scene fits, in its merged-trace form for
    // small triangle scenes; else the multi-pass wavefront (k_shade, then k_trace streaming the
    // scene through LDS tiles).  Two-level scenes (C4) take the merged kernel with the wave's
    // own BVH walk.  Direct / Normal over an LDS-resident scene: pixel-parallel sample chains
    // (pixel.hip).  Speculative sample starts serve the merged schedule's 16-slot and tail
    // launches (spec.hip).
    R.two_level = !(p->flags & (XRT_FLAG_WAVEFRONT | XRT_FLAG_NO_MERGED)) && use_step_bvh(P);
    R.pixel = !R.two_level && !(p->flags & (XRT_FLAG_WAVEFRONT | XRT_FLAG_NO_PIXEL)) && use_pixel(P);
    R.fused = R.two_level || (!(p->flags & XRT_FLAG_WAVEFRONT) && step_lds_bytes(P) != 0);
    R.merged = R.two_level || (R.fused && !(p->flags & XRT_FLAG_NO_MERGED) && use_step_merged(P));
    R.step_tri = R.fused && !R.merged && use_step_tri(P);
    R.spec = R.merged && !R.two_level && !(p->flags & XRT_FLAG_NO_SPEC) && use_step_spec(P);
    R.camlist = R.spec && !exp_env("XRT_NO_CAMLIST");
    // Direct (under XRT_FLAG_NO_PIXEL) keeps tracing its empty pixels: its miss adds the
    // background per sample, an in-order float sum with no closed form
    R.elide = XRT_CAM_ELIDE && !exp_env("XRT_NO_ELIDE") && R.merged && !R.two_level && !R.pixel &&
              p->integrator == XRT_INTEGRATOR_GI && p->max_depth >= 1 && p->spp >= 1 && P.n_tris <= 64;
    // WhittedIntegrator has one schedule, whatever the schedule flags say (render_impl has
    // refused the scenes it cannot hold): one wave per pixel, one lane per sample (whitted.hip),
    // over the LDS scene when it fits, else — XRT_FLAG_WHITTED_BVH — through the triangle BVH
    R.whitted = p->integrator == XRT_INTEGRATOR_WHITTED;
    R.whitted_bvh = R.whitted && (p->flags & XRT_FLAG_WHITTED_BVH) && !use_whitted(P) && use_whitted_bvh(P);
    if (R.whitted) R.pixel = true, R.two_level = R.merged = R.step_tri = R.spec = R.camlist = R.elide = false;
    R.schedule = R.whitted_bvh ? XRT_SCHED_WHITTED_BVH
                 : R.whitted   ? XRT_SCHED_WHITTED
                 : R.pixel     ? XRT_SCHED_PIXEL
                 : !R.fused    ? XRT_SCHED_WAVEFRONT
                 : R.two_level ? XRT_SCHED_STEP_BVH
                 : R.merged    ? XRT_SCHED_STEP_MERGED
                 : R.step_tri  ? XRT_SCHED_STEP_TRI
                               : XRT_SCHED_STEP;
    // live-list partitions (a multiple of the 8 XCDs): every wave appends to its partition's
    // counters once per launch, so more partitions mean less atomic contention (64 -> 256:
    // C4 -14%, C2 -4.5%).  The merged schedule (64 segments per launch) is fastest with
    // >= 2048 slots per partition (at most 256), the per-segment ones with >= 512 (at most
    // kMaxParts): C3 -8%, C4 -4% over 256
    const size_t cap = R.merged ? 256 : kMaxParts, per = R.merged ? 2048 : kPartMinSlots;
    R.n_part = (uint32_t)std::min<size_t>(cap, std::max<size_t>(1, n / per));
    if (R.n_part >= 8) R.n_part &= ~7u;
    R.part_cap = (uint32_t)((n + R.n_part - 1) / R.n_part);
    // the merged schedule's full-wave launches in partition groups (step_groups.h): one-level
    // scenes; the two-level kernel's launches are not measured in groups and stay whole
    R.groups = R.merged && !R.two_level && !R.pixel && !R.whitted && !(p->flags & XRT_FLAG_NO_OVERLAP)
                   ? step_groups_for(R.n_part, XRT_STEP_GROUPS)
                   : 1u;
    // pixels interleaved across slots (slot_map.h), so the waves of a launch cost about alike: the
    // merged schedule — one-level shards from kSlotInterleaveMin slots on, two-level ones that start in
    // the whole-wave layout (the sizes measured, tuning.h).  The flags force it on, for a merged render
    // of any size, or off; every other schedule's kernels know the row-major map only
    const bool can_interleave = R.merged && !R.pixel && !R.whitted && !(p->flags & XRT_FLAG_NO_INTERLEAVE);
    const bool auto_interleave = XRT_SLOT_INTERLEAVE && (R.two_level ? n >= kBvhLive64 && step_merged_spw(P, n) == 64
                                                                     : n >= kSlotInterleaveMin);
    const char* ei = exp_env("XRT_INTERLEAVE");   // experiment builds only: 1 as XRT_FLAG_INTERLEAVE, 0 as NO_INTERLEAVE
    const bool want_interleave = ei ? std::atoi(ei) != 0 : ((p->flags & XRT_FLAG_INTERLEAVE) || auto_interleave);
    R.slot_mul = can_interleave && want_interleave ? slot_multiplier((uint32_t)n) : 0u;
    // segments per slot per step launch: kMergedVisits / kStepVisits unless the caller sets
    // visits_per_launch (results do not depend on it)
    const uint32_t draws = step_merged_draws(P);
    const char* ev = exp_env("XRT_VISITS");   // experiment builds only
    R.step_visits = ev                             ? (uint32_t)std::atoi(ev)
                    : p->visits_per_launch          ? p->visits_per_launch
                    : R.merged                      ? std::min<uint32_t>(kMergedVisits, (kMT - draws) / draws)
                    : (R.volumetric && kVptEvents) ? kVptEventVisits
                                                    : kStepVisits;
    // the whole-wave phase in block-owned chunks (host/step_chunks.cpp has the rule): one-level
    // renders traced by pair passes that start in whole waves and are interleaved by the rule above,
    // with launch geometry left to the library and samples enough for two passes per launch; the flags
    // force it for any such render that starts in whole waves, or forbid it
    {
        ChunkRule cr{};
        cr.one_level_merged = R.merged && !R.two_level && !R.pixel && !R.whitted && !R.mom && !exp_env("XRT_LANE_TRACE") &&
                              R.step_visits >= 1 && R.step_visits <= 255;
        cr.starts_whole_waves = cr.one_level_merged && step_merged_spw(P, n) == 64;
        cr.interleaved = can_interleave && auto_interleave && R.slot_mul != 0;
        cr.force = (p->flags & XRT_FLAG_CHUNKS) != 0, cr.forbid = (p->flags & XRT_FLAG_NO_CHUNKS) != 0;
        cr.visits_req = ev ? 1u : p->visits_per_launch, cr.spw_req = p->slots_per_wave;
        cr.spp = p->spp, cr.max_depth = p->max_depth, cr.visits = R.step_visits;
        cr.class_cap = chunk_class_cap(R.n_part, R.part_cap);
        const char* eq = exp_env("XRT_CHUNK_Q");   // experiment builds only
        cr.pass_cap = eq ? (uint32_t)std::min(255, std::max(1, std::atoi(eq))) : XRT_CHUNK_PASSES;
        R.chunk_passes = chunk_plan(cr);
        R.chunk_class_cap = cr.class_cap;
        R.chunk_forced = cr.force;
    }
    // k_step_spec reads up to kSpecDraws words past the cursor per visit: fewer visits per launch
    // (with XRT_SPEC_TWIST it twists in-loop instead: XRT_SPEC_VISITS visits unless the caller sets them)
    R.spec_visits = !R.spec          ? 0
                    : XRT_SPEC_TWIST ? ((ev || p->visits_per_launch) ? R.step_visits : XRT_SPEC_VISITS)
                                     : std::min<uint32_t>(R.step_visits, (kMT - kSpecDraws) / kSpecDraws);
    // a slot's ring is twisted at the end of a launch when fewer words are left than the next
    // launch can draw: the merged kernel draws at most step_merged_draws per segment and
    // checks it; k_step / k_step_tri check kRngVisit per visit
    R.rng_keep = R.spec && !XRT_SPEC_TWIST
                     ? std::max(R.step_visits * draws + draws, R.spec_visits * kSpecDraws + kSpecDraws)
                 : R.merged                     ? R.step_visits * draws + draws
                 : (R.volumetric && kVptEvents) ? R.step_visits * kVptEventDraws + kRngVisit
                                                : R.step_visits * kVisitDraws + kRngVisit;
    // the merged schedule polls every launch and runs at most 3 launches ahead of the last
    // retired poll, so the layout and grid it chooses per launch follow the live count closely
    R.poll_every = R.merged ? 1 : R.fused ? 4 : 16;
    R.ahead = R.merged ? 3 : R.fused ? 16 : 64;
    // GI/Direct: at most max_depth + 1 shade passes per sample; VPT walks are unbounded
    // (null collisions, suspensions), so only the live-slot poll ends the loop there.
    R.cap_iters = R.volumetric ? (uint64_t)p->spp * 100000ull + 1000000ull
                               : (uint64_t)p->spp * (p->max_depth + 2) + 16;
    return R;
}

namespace {

// Asynchronous termination polling.  Every `every` loop iterations the live counters that
// iteration wrote are copied into one of the context's 8 pinned slots, with an event behind
// the copy.  Polls are retired in order: without blocking once their event has fired, by
// waiting once the host is `ahead` iterations past one.  Retired polls give `done` (no live
// slot left) and the live counts the merged schedule chooses its layout and grid by (upper
// bounds: paths only finish).  An iteration launched in G partition groups (run_fused) is polled
// without a barrier between the groups: each group copies the counters on its own stream, in
// order behind its launch, into pinned slots of its own, of which the host reads that group's
// partitions only, and the poll is retired when every group's event has fired.  The live counts
// are taken over all groups, so they keep their whole-GPU meaning.
struct LivePoll {
    xrt_ctx* c;
    uint32_t n_part;
    uint64_t every, ahead;
    bool part_max;            // follow the fullest partition too (merged schedule, layout not forced)
    uint64_t live_hint;       // live slots at the last retired poll
    uint32_t live_part_max;   // ... in the fullest partition
    bool done = false;
    uint64_t retired = 0;     // polls retired so far
    struct Pending { uint64_t it; int slot; uint32_t groups; bool parts; };   // parts: the counters are per partition (part_max when issued)
    std::vector<Pending> pending;
    int issued = 0;

    // after iteration `it`, whose launches left the live counts in `live` (device); groups > 1: one
    // launch per partition group, on c->group_stream
    int after(uint64_t it, const uint32_t* live, uint32_t groups = 1) {
        if (it % every == every - 1) {
            const int ps = issued++ % 8;
            for (uint32_t g = 0; g < groups; ++g) {
                hipStream_t st = groups > 1 ? c->group_stream[g] : c->stream;
                HIPCHK(c, hipMemcpyAsync(c->h_poll + (ps * kMaxStepGroups + g) * kMaxParts, live, n_part * 4,
                                         hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipEventRecord(c->poll_ev[ps][g], st));
            }
            pending.push_back({it, ps, groups, part_max});
        }
        while (!pending.empty()) {
            const Pending q = pending.front();
            const bool must_wait = it - q.it >= ahead;
            bool fired = true;
            for (uint32_t g = 0; g < q.groups && fired && !must_wait; ++g)
                fired = hipEventQuery(c->poll_ev[q.slot][g]) == hipSuccess;
            if (!fired) break;
            for (uint32_t g = 0; g < q.groups; ++g) HIPCHK(c, hipEventSynchronize(c->poll_ev[q.slot][g]));
            const uint32_t* h0 = c->h_poll + (size_t)q.slot * kMaxStepGroups * kMaxParts;
            uint64_t alive = 0;
            uint32_t pmax = 0;
            for (uint32_t k = 0; k < n_part; ++k) {
                const uint32_t v = h0[step_group_of(q.groups, k) * kMaxParts + k];
                alive += v, pmax = std::max(pmax, v);
            }
            ++retired;
            if (alive == 0) done = true;
            if (alive < live_hint) {
                live_hint = alive;
                if (part_max && q.parts) live_part_max = std::max(1u, pmax);
            }
            pending.erase(pending.begin());
            if (done) break;
        }
        return XRT_OK;
    }
};

}  // namespace

// k_seed, then the slots' first samples: k_pixel renders them outright; every other schedule
// twists each slot's ring (the refill k_seed requested).  Last, the device copy of the
// parameters for the kernels that read them from memory.
int seed_paths(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, LaunchTimer& T) {
    HIPCHK(c, T.launch(XRT_K_SEED, [&] { return launch_seed(P, L.list[0], L.counts(0), L.counts(1), L.req(0), c->stream); }));
    if (R.pixel) {
        // every pixel of the shard in one persistent launch; the pixel counter is a stats word
        // (zeroed with them)
        uint32_t* work = reinterpret_cast<uint32_t*>(P.stats + kStatsWork);
        const hipError_t e = T.launch(XRT_K_STEP, [&] {
            return R.whitted_bvh ? launch_whitted_bvh(P, work, c->stream, R.mom)
                   : R.whitted   ? launch_whitted(P, work, c->stream, R.mom)
                                 : launch_pixel(P, work, c->stream);
        });
        if (e != hipSuccess) return hip_err(c, e, R.whitted_bvh ? "k_whitted_bvh" : R.whitted ? "k_whitted" : "k_pixel");
    } else {
        HIPCHK(c, T.launch(XRT_K_REFILL, [&] {
            return R.merged ? launch_refill_merged(P, L.req(0), L.req(1), c->stream)
                            : launch_refill(P, L.req(0), L.req(1), c->stream);
        }));
        // the camera lists now, not before the first speculative launch: the pixels they prove
        // empty are finished before any step launch loads them
        if (R.elide) HIPCHK(c, T.launch(XRT_K_SEED, [&] { return launch_camlist(P, true, c->stream); }));
    }
    HIPCHK(c, hipMemcpyAsync(c->kparams.p, &P, sizeof(KParams), hipMemcpyHostToDevice, c->stream));
    return XRT_OK;
}

namespace {

// The fused schedules' loop: one step launch per iteration over three rotating counter
// arrays — round i reads counts(i % 3), appends to counts((i + 1) % 3) and clears
// counts((i + 2) % 3) for round i + 1.  Every step kernel twists its slots' rings in-line at
// the end of the launch.  The merged schedule chooses its slots-per-wave layout every launch
// from the live count of the last retired poll, so a frame's tail, where few slots remain,
// runs with more lanes per slot, and sizes the grid by the fullest partition's
// live count instead of its capacity.  Results never depend on the layout.
//
// While the merged schedule runs whole waves (64 slots each) and the plan has partition groups
// (RenderPlan::groups, step_groups.h), an iteration is one launch per group, each on the group's
// own stream, so one group's last waves do not hold back the next round of the others.  All of
// them are launches of the same iteration: the list ping-pong and the counter rotation stay
// common, each launch reading, appending to and clearing its own group's partitions.  The group
// streams leave c->stream by an event before the first such iteration and join it again, by
// events, when the layout leaves 64 slots per wave, when the loop ends and when a call fails;
// from the join on the loop runs as it does without groups.  Nothing waits on the device.
class StepGroupStreams {
  public:
    StepGroupStreams(xrt_ctx* c, LaunchTimer& T, uint32_t groups) : c_(c), T_(T), groups_(groups) {}
    ~StepGroupStreams() { (void)join(); }   // an error path: bring the streams back all the same
    bool forked() const { return forked_; }
    // the group streams (made with the context's first grouped render) wait for c->stream's work so far
    int fork() {
        if (forked_) return XRT_OK;
        for (uint32_t g = 0; g < groups_; ++g) {
            if (!c_->group_stream[g]) HIPCHK(c_, hipStreamCreateWithFlags(&c_->group_stream[g], hipStreamNonBlocking));
            if (!c_->join_ev[g]) HIPCHK(c_, hipEventCreateWithFlags(&c_->join_ev[g], hipEventDisableTiming));
        }
        if (!c_->fork_ev) HIPCHK(c_, hipEventCreateWithFlags(&c_->fork_ev, hipEventDisableTiming));
        T_.span_begin(XRT_K_STEP);
        HIPCHK(c_, hipEventRecord(c_->fork_ev, c_->stream));
        forked_ = true;   // from here on a join is owed, whatever fails
        for (uint32_t g = 0; g < groups_; ++g) HIPCHK(c_, hipStreamWaitEvent(c_->group_stream[g], c_->fork_ev, 0));
        return XRT_OK;
    }
    // c->stream waits for every group stream's work so far
    int join() {
        if (!forked_) return XRT_OK;
        forked_ = false;
        hipError_t first = hipSuccess;
        for (uint32_t g = 0; g < groups_; ++g) {
            hipError_t e = hipEventRecord(c_->join_ev[g], c_->group_stream[g]);
            if (e == hipSuccess) e = hipStreamWaitEvent(c_->stream, c_->join_ev[g], 0);
            if (first == hipSuccess) first = e;
        }
        T_.span_end();
        return first == hipSuccess ? XRT_OK : hip_err(c_, first, "joining the step group streams");
    }

  private:
    xrt_ctx* c_;
    LaunchTimer& T_;
    uint32_t groups_;
    bool forked_ = false;
};

}  // namespace

// The chunk buffer of a render whose plan has the chunk phase (launch.h ChunkBufs), and the chunks
// themselves from the seeded lists: timed with the seeding.  The host then reads the header back (one
// wait for the seeding per frame): the chunks that hold a slot, and the grid of the phase's launches
// from them, 8 blocks per chunk of the fullest class, at most 8 * kChunkClassBlocks.  A phase taken by
// the rule, not forced, runs only where no block owns more than one chunk (at most kChunkClassBlocks
// chunks per class), which is what has been measured; otherwise B.blocks = 0 and the
// grouped schedule runs from the seeded lists, which the build has not touched.
int build_chunks(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, LaunchTimer& T, ChunkBufs& B) {
    const size_t chunks = 8u * (size_t)R.chunk_class_cap, head = kChunkHdrWords + kMaxParts + 2 * chunks;
    const int rc = ensure(c, c->chunks, (head + 2 * chunks * kChunkSlots) * sizeof(uint32_t));
    if (rc) return rc;
    B.hdr = as<uint32_t>(c->chunks), B.part_live = B.hdr + kChunkHdrWords, B.cnt = B.part_live + kMaxParts;
    B.seg = B.hdr + head, B.class_cap = R.chunk_class_cap;
    HIPCHK(c, hipMemsetAsync(B.hdr, 0, head * sizeof(uint32_t), c->stream));
    HIPCHK(c, T.launch(XRT_K_SEED, [&] { return launch_chunks_build(P, B, L.list[0], L.counts(0), c->stream); }));
    uint32_t head_words[kChunkHdrWords];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(head_words, B.hdr, sizeof(head_words), hipMemcpyDeviceToHost));
    uint32_t max_nx = 0;
    B.chunks = 0;
    for (uint32_t x = 0; x < 8; ++x) B.chunks += head_words[x], max_nx = std::max(max_nx, head_words[x]);
    B.blocks = 8u * chunk_class_blocks(max_nx);
    if (!R.chunk_forced && max_nx > kChunkClassBlocks) B.blocks = 0;
    return XRT_OK;
}

namespace {

// The whole-wave phase in block-owned chunks, ahead of run_fused's loop and counted as its first
// iterations: launch `it` adds the live slots it leaves to counts((it + 1) % 3) and clears
// counts((it + 2) % 3), the rotation of the loop, so LivePoll reads it as any round (the sums are per
// block, not per partition: the fullest partition is not followed here).  The host stays one launch
// ahead of the last retired poll, a launch being several rounds long.  The phase ends when a retired
// poll finds fewer live slots than whole waves are worth (kMergedLive64), or none; then
// k_chunks_scatter puts the live slots back on the partition lists, as round `it` expects them.
int run_chunks(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, const ChunkBufs& B, LaunchTimer& T,
               LivePoll& poll, uint64_t& it) {
    const KParams* dP = as<KParams>(c->kparams);
    const bool part_max = poll.part_max;
    const uint64_t ahead = poll.ahead;
    poll.part_max = false, poll.ahead = 1;
    int rc = XRT_OK;
    for (it = 0; it < R.cap_iters && !poll.done; ++it) {
        if (poll.retired && poll.live_hint < kMergedLive64) break;
        T.step_live.push_back(poll.live_hint);
        T.S.layout_launches[0]++;
        const hipError_t e = T.launch(XRT_K_STEP, [&] {
            return launch_step_merged_chunks(P, dP, c->step_objs, B, L.counts((it + 1) % 3), L.counts((it + 2) % 3),
                                             R.step_visits, R.chunk_passes, (uint32_t)it, c->stream);
        });
        if (e != hipSuccess) return hip_err(c, e, "k_step_merged_chunks");
        if ((rc = poll.after(it, L.counts((it + 1) % 3)))) break;
    }
    poll.part_max = part_max, poll.ahead = ahead;
    if (rc || poll.done) return rc;
    HIPCHK(c, hipMemsetAsync(L.counts(it % 3), 0, P.n_part * sizeof(uint32_t), c->stream));
    HIPCHK(c, T.launch(XRT_K_SEED, [&] { return launch_chunks_scatter(P, B, L.list[it & 1], L.counts(it % 3), c->stream); }));
    return XRT_OK;
}

int run_fused(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, const ChunkBufs& B, LaunchTimer& T,
              LivePoll& poll, uint64_t& it) {
    const KParams* dP = as<KParams>(c->kparams);
    const uint32_t blocks = P.n_part * ((P.part_cap + 255) / 256);   // k_step, k_step_tri: one entry per thread
    // built before the first launch that reads them (seed_paths has when it elides), timed with the seeding
    bool camlist_pending = R.camlist && !R.elide;
    StepGroupStreams GS(c, T, R.groups);
    it = 0;
    if (R.chunk_passes && B.blocks) {   // the group streams fork after it, if whole waves are still worth running
        const int rc = run_chunks(c, P, R, L, B, T, poll, it);
        if (rc) return rc;
    }
    for (; it < R.cap_iters && !poll.done; ++it) {
        const uint32_t *list = L.list[it & 1], *ci = L.counts(it % 3);
        uint32_t *out = L.list[~it & 1], *co = L.counts((it + 1) % 3), *cz = L.counts((it + 2) % 3);
        const uint32_t spw = R.merged ? step_merged_spw(P, poll.live_hint) : 0;
        const uint32_t groups = spw == 64 ? R.groups : 1u;
        // one entry per timed step entry: a span of grouped rounds is one (the live hint it began with)
        if (groups == 1 || !GS.forked()) T.step_live.push_back(poll.live_hint);
        if (R.merged) T.S.layout_launches[spw == 64 ? 0 : spw == 32 ? 1 : spw == 16 ? 2 : spw == 8 ? 3 : 4] += groups;
        int rc;
        if (groups > 1) {
            if ((rc = GS.fork())) return rc;
            for (uint32_t g = 0; g < groups; ++g) {
                const hipError_t e = launch_step_merged(P, dP, c->step_objs, list, ci, out, co, cz, L.req(1), R.step_visits,
                                                        poll.live_hint, poll.live_part_max, groups, g, c->group_stream[g], R.mom);
                if (e != hipSuccess) return hip_err(c, e, "k_step");
            }
            T.S.launches[XRT_K_STEP] += groups;
            if ((rc = poll.after(it, co, groups))) return rc;
            continue;
        }
        if ((rc = GS.join())) return rc;
        // speculative starts in the group layouts (4 lanes per slot; 16 in the tail; 8 when forced)
        const bool spec_now = R.spec && P.camlist && (spw == 16 || spw == 8 || (XRT_SPEC_TAIL && spw == 4)) &&
                              step_merged_group(P, spw) * spw == 64;
        if (spec_now) T.S.spec_launches++;
        if (spec_now && camlist_pending) {
            camlist_pending = false;
            HIPCHK(c, T.launch(XRT_K_SEED, [&] { return launch_camlist(P, false, c->stream); }));
        }
        const hipError_t e = T.launch(XRT_K_STEP, [&] {
            if (spec_now)
                return launch_step_spec(P, dP, list, ci, out, co, cz, R.spec_visits, poll.live_part_max, spw, c->stream);
            if (R.merged)
                return launch_step_merged(P, dP, c->step_objs, list, ci, out, co, cz, L.req(1), R.step_visits,
                                          poll.live_hint, poll.live_part_max, 1, 0, c->stream, R.mom);
            return launch_step(P, dP, list, ci, out, co, cz, L.req(1), R.step_visits, blocks, poll.live_hint, R.step_tri,
                               c->stream, R.mom);
        });
        if (e != hipSuccess) return hip_err(c, e, "k_step");
        if ((rc = poll.after(it, co))) return rc;
    }
    return GS.join();
}

// The wavefront loop: k_shade reads list[i & 1] and appends the surviving slots to the other
// list (two alternating counter arrays; it twists its slots' rings in-line), k_trace traces
// them and clears the counters k_shade read, and two-level scenes walk the BVH for the rays
// the trace queued.
int run_wavefront(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, LaunchTimer& T, LivePoll& poll,
                  uint64_t& it) {
    const uint32_t blocks = P.n_part * ((P.part_cap + 255) / 256);   // one entry per thread
    for (it = 0; it < R.cap_iters && !poll.done; ++it) {
        const int cur = (int)(it & 1), nxt = cur ^ 1;
        hipError_t e = T.launch(XRT_K_SHADE, [&] {
            return launch_shade(P, L.list[cur], L.counts(cur), L.list[nxt], L.counts(nxt), L.req(1), blocks, c->stream,
                                R.mom);
        });
        if (e != hipSuccess) return hip_err(c, e, "k_shade");
        e = T.launch(XRT_K_TRACE, [&] {
            return launch_trace(P, L.list[nxt], L.counts(nxt), L.counts(cur), blocks, c->stream, false);
        });
        if (e != hipSuccess) return hip_err(c, e, "k_trace");
        if (P.two_level && P.bvh_node && P.scene_kind == SCN_TRI) {
            e = T.launch(XRT_K_DEEP, [&] { return launch_trace_deep(P, c->stream); });
            if (e != hipSuccess) return hip_err(c, e, "k_trace_deep4");
        }
        const int rc = poll.after(it, L.counts(nxt));
        if (rc) return rc;
    }
    return XRT_OK;
}

}  // namespace

// the device's stats words into xrt_stats (and the counters of experiment builds to stderr)
int read_stats(xrt_ctx* c, const KParams& P, xrt_stats& S) {
    unsigned long long hs[48] = {0};
    HIPCHK(c, hipMemcpy(hs, P.stats, 48 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (XRT_PHASE_CLOCK)   // experiment builds: k_step_spec's visit phases (shader-clock cycles summed over waves)
        std::fprintf(stderr, "[xrt] spec phase cycles head %llu trace %llu candidates %llu end-test %llu shading %llu"
                     " moves %llu cursor+reload %llu launch %llu\n", hs[40], hs[41], hs[42], hs[43], hs[44], hs[45],
                     hs[46], hs[47]);
    if (hs[38])   // experiment builds (-DXRT_EXPERIMENTS): BVH walk counters
        std::fprintf(stderr, "[xrt] deep rays %llu node steps %llu wave iterations %llu max wave iterations %llu"
                     " in-wave walks %llu\n", hs[38], hs[39], hs[37], hs[36], hs[35]);
    S.segments = hs[0], S.shadow_rays = hs[1], S.draws = hs[2], S.rejected = hs[3], S.stalled = hs[4];
    S.rng_twists = hs[7];
    S.pix_windows = hs[kStatsPix], S.pix_stride4 = hs[kStatsPix + 1], S.pix_frustum = hs[kStatsPix + 2];
    S.pix_frustum_overflow = hs[kStatsPix + 3], S.pix_shadow_list = hs[kStatsPix + 4];
    S.pix_shadow_overflow = hs[kStatsPix + 5], S.pix_flushes = hs[kStatsPix + 6];
    S.whit_rays = hs[kStatsWhit], S.whit_depth_cut = hs[kStatsWhit + 1], S.whit_refract = hs[kStatsWhit + 2];
    S.whit_tir = hs[kStatsWhit + 3];
    return XRT_OK;
}

// the plan's share of the parameters: partitions, refill threshold and slot map, the live lists and the
// request list behind them, the two-level queues and, where the plan builds them, the camera lists
int bind_plan(xrt_ctx* c, KParams& P, const RenderPlan& R, LiveLists& L) {
    P.n_part = R.n_part, P.part_cap = R.part_cap, P.rng_keep = R.rng_keep, P.slot_mul = R.slot_mul;
    const size_t lcap = (size_t)P.n_part * P.part_cap;
    L = LiveLists{{as<uint32_t>(c->lists), as<uint32_t>(c->lists) + lcap}, as<uint32_t>(c->counts)};
    P.req = as<uint32_t>(c->lists) + 2 * lcap;
    int rc;
    if ((rc = setup_deep(c, P))) return rc;
    if (R.camlist) {   // the pixels' camera-ray triangle lists: k_step_spec's candidates
        if ((rc = ensure(c, c->camlist, (size_t)P.n_slots * sizeof(uint4)))) return rc;
        P.camlist = as<uint4>(c->camlist);
    }
    return XRT_OK;
}

// the path work of a seeded (or resumed) render: the plan's loop until a poll finds no live slot or the
// iteration cap is reached; a pixel-parallel plan has none.  it: the iterations run; done: a poll saw
// the lists empty (else check_drained, once the stream is synchronised)
int run_paths(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, const ChunkBufs& CB, LaunchTimer& T,
              uint64_t& it, bool& done) {
    LivePoll poll{c, P.n_part, R.poll_every, R.ahead, R.merged && !P.spw_req, P.n_slots, P.part_cap};
    it = 0;
    int rc = XRT_OK;
    if (!R.pixel) rc = R.fused ? run_fused(c, P, R, L, CB, T, poll, it) : run_wavefront(c, P, R, L, T, poll, it);
    done = R.pixel || poll.done;
    return rc;
}

// the iteration cap was reached without observing an empty list: verify
int check_drained(xrt_ctx* c, const KParams& P, const RenderPlan& R, const LiveLists& L, uint64_t it) {
    uint32_t left[kMaxParts] = {0};
    HIPCHK(c, hipMemcpy(left, L.counts(R.fused ? it % 3 : it & 1), P.n_part * 4, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < P.n_part; ++k)
        if (left[k] != 0) return set_err(c, XRT_ERR_HIP, "iteration cap reached with live paths");
    return XRT_OK;
}

// what xrt_stats says about the plan and its run
void plan_stats(const KParams& P, const RenderPlan& R, uint64_t it, xrt_stats& S) {
    S.iterations = it;
    S.schedule = (uint64_t)R.schedule;
    S.partitions = P.n_part;
    if (R.fused && !R.pixel) S.visits_per_launch = R.step_visits;
    if (R.merged && !R.pixel) {
        S.slots_per_wave = step_merged_spw(P, P.n_slots);   // the layout of the first launch (every launch's: layout_launches)
        S.group_lanes = step_merged_group(P, S.slots_per_wave);
    }
}

int render_impl(xrt_ctx* c, const xrt_render_params* p, float* d_out, float* h_out, xrt_stats* st, int wait,
                hipStream_t wait_stream, float* d_var, ChunkProbe* probe) {
    const auto t_start = std::chrono::steady_clock::now();
    int rc = check_render(c, p);
    if (rc) return rc;
    // A variance render is this render with its plan forced to the wavefront schedule (Whitted has
    // one schedule anyway): no other schedule flag and no launch geometry reaches the plan.  Under
    // XRT_FLAG_VAR_FUSED it is this render without speculative starts and pixel-parallel chains,
    // whose kernels have no moments build: the plan is xrt_render's for those flags.
    xrt_render_params forced;
    if (d_var) {
        if ((rc = check_render_var(c, p))) return rc;
        forced = *p;
        if ((p->flags & XRT_FLAG_VAR_FUSED) && !(p->flags & XRT_FLAG_WAVEFRONT) && p->integrator != XRT_INTEGRATOR_WHITTED) {
            forced.flags = (p->flags & ~XRT_FLAG_VAR_FUSED) | XRT_FLAG_NO_SPEC | XRT_FLAG_NO_PIXEL;
        } else {
            forced.flags = (p->flags & (XRT_FLAG_TIMING | XRT_FLAG_WHITTED_BVH)) | XRT_FLAG_WAVEFRONT;
            forced.slots_per_wave = forced.visits_per_launch = 0;
        }
        p = &forced;
    }
    end_progressive(c);   // the slots are seeded anew
    if ((rc = order_after(c, wait, wait_stream, false))) return rc;
    const size_t n = (size_t)shard_rows(p->height, p->shard_index, p->shard_count) * p->width;
    const size_t npix = (size_t)p->width * p->height;
    if (n == 0) return render_empty_shard(c, p, d_out, h_out, d_var, st, t_start);

    // buffers, parameters, plan
    if ((rc = grow_slots(c, n)) || (!d_out && (rc = ensure(c, c->fb, npix * 3 * sizeof(float)))) ||
        (d_var && (rc = ensure(c, c->mom, n * sizeof(float2)))))
        return rc;
    float* fb = d_out ? d_out : as<float>(c->fb);   // the caller's device image, or the context's own
    KParams P = render_params(c, p, n, fb);
    if (p->integrator == XRT_INTEGRATOR_WHITTED && !use_whitted(P)) {
        if (!(p->flags & XRT_FLAG_WHITTED_BVH))
            return set_err(c, XRT_ERR_UNSUPPORTED,
                           "WhittedIntegrator needs a scene that fits the LDS-resident scene carve (not a two-level scene)");
        if (!use_whitted_bvh(P))
            return set_err(c, XRT_ERR_UNSUPPORTED,
                           "WhittedIntegrator with XRT_FLAG_WHITTED_BVH: the scene neither fits the LDS-resident scene "
                           "carve nor has a triangle BVH (a large sphere-only or mixed scene)");
    }
    const RenderPlan R = plan_render(P, p, d_var ? as<float2>(c->mom) : nullptr);
    if (!R.pixel && R.rng_keep > kMT) return set_err(c, XRT_ERR_INVALID, "visits_per_launch too large for the RNG ring");
    if (probe) {
        probe->passes = R.chunk_passes;
        if (!R.chunk_passes) return XRT_OK;
    }
    LiveLists L{};
    if ((rc = bind_plan(c, P, R, L))) return rc;
    xrt_stats S{};
    S.path_slots = n;
    S.samples = (uint64_t)n * p->spp;
    LaunchTimer T{c, S, (p->flags & XRT_FLAG_TIMING) != 0, {}, {}};

    // seed
    if (!(p->flags & XRT_FLAG_ACCUMULATE))
        HIPCHK(c, hipMemsetAsync(fb, 0, npix * 3 * sizeof(float), c->stream));
    else if (h_out)   // the caller's Image is the accumulator (Src/renderer.cpp:75)
        HIPCHK(c, hipMemcpyAsync(fb, h_out, npix * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (d_var) HIPCHK(c, hipMemsetAsync(d_var, 0, npix * sizeof(float), c->stream));   // outside the shard: +0
    HIPCHK(c, hipMemsetAsync(P.stats, 0, 512, c->stream));
    // the fused kernels' moments builds only add to the records (k_shade zeroes a record in the slot's
    // first visit), and a pixel k_camlist retires is never loaded by one: its record stays {+0, +0}
    if (R.mom && R.fused && !R.pixel) HIPCHK(c, hipMemsetAsync(R.mom, 0, n * sizeof(float2), c->stream));
    if ((rc = seed_paths(c, P, R, L, T))) return rc;
    ChunkBufs CB{};
    if (R.chunk_passes && (rc = build_chunks(c, P, R, L, T, CB))) return rc;
    if (probe) {   // xrt_test_chunk_plan: the chunks as built, nothing rendered
        const uint32_t cap = 8u * CB.class_cap;
        std::vector<uint32_t> cnt(2 * (size_t)cap);
        HIPCHK(c, hipMemcpy(cnt.data(), CB.cnt, cnt.size() * 4, hipMemcpyDeviceToHost));   // build_chunks has waited
        probe->chunks = CB.chunks, probe->blocks = CB.blocks, probe->cap = cap;   // blocks 0: bounded off, the grouped schedule runs
        for (uint32_t q = 0; q < cap && q < probe->n_sizes; ++q) probe->sizes[q] = cnt[2 * q] + cnt[2 * q + 1];
        return XRT_OK;
    }

    // run, finish
    uint64_t it = 0;
    bool done = false;
    if ((rc = run_paths(c, P, R, L, CB, T, it, done))) return rc;
    HIPCHK(c, T.launch(XRT_K_FINISH, [&] {   // a variance render's plane counts as part of the finish
        const hipError_t e = launch_finish(P, c->stream);
        return e != hipSuccess || !R.mom ? e : launch_finish_var(P, R.mom, d_var, c->stream);
    }));
    HIPCHK(c, hipStreamSynchronize(c->stream));
#if XRT_PHASE_CLOCK
    HIPCHK(c, wave_clock_dump(exp_env("XRT_WAVE_CLOCK_OUT"), c->stream));
#endif
    if (!done && (rc = check_drained(c, P, R, L, it))) return rc;

    // stats
    if ((rc = read_stats(c, P, S))) return rc;
    plan_stats(P, R, it, S);
    T.read_out();
    if (h_out) HIPCHK(c, hipMemcpy(h_out, fb, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    S.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (st) *st = S;
    return XRT_OK;
}

}  // namespace xrt

using namespace xrt;

extern "C" {

int xrt_render(xrt_ctx* c, const xrt_render_params* p, float* rgb_out, xrt_stats* st) {
    if (!rgb_out) return set_err(c, XRT_ERR_INVALID, "null output");
    if (c && !c->subs.empty()) return render_multi(c, p, nullptr, rgb_out, st, 0, nullptr);
    return render_impl(c, p, nullptr, rgb_out, st);
}

int xrt_render_device(xrt_ctx* c, const xrt_render_params* p, float* d_rgb_out, xrt_stats* st) {
    if (!d_rgb_out) return set_err(c, XRT_ERR_INVALID, "null output");
    if (c && !c->subs.empty()) return render_multi(c, p, d_rgb_out, nullptr, st, 1, nullptr);
    return render_impl(c, p, d_rgb_out, nullptr, st, 1);
}

int xrt_render_device_after(xrt_ctx* c, const xrt_render_params* p, float* d_rgb_out, void* hip_stream,
                            xrt_stats* st) {
    if (!d_rgb_out) return set_err(c, XRT_ERR_INVALID, "null output");
    if (c && !c->subs.empty()) return render_multi(c, p, d_rgb_out, nullptr, st, 2, (hipStream_t)hip_stream);
    return render_impl(c, p, d_rgb_out, nullptr, st, 2, (hipStream_t)hip_stream);
}

// the slot -> pixel map the render of p would use, through the kernels' own device function
int xrt_test_slot_map(xrt_ctx* c, const xrt_render_params* p, uint32_t* out) {
    c = first_device(c);
    if (!c || !p || !out) return XRT_ERR_INVALID;
    int rc = check_render(c, p);
    if (rc) return rc;
    const size_t n = (size_t)shard_rows(p->height, p->shard_index, p->shard_count) * p->width;
    if (n == 0) return XRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf d;
    if ((rc = ensure(c, d, n * sizeof(uint32_t)))) return rc;
    KParams P = render_params(c, p, n, nullptr);
    P.slot_mul = plan_render(P, p, nullptr).slot_mul;
    hipError_t e = launch_test_slot_map(P, as<uint32_t>(d), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    free_buf(d);
    return e == hipSuccess ? XRT_OK : hip_err(c, e, "xrt_test_slot_map");
}

// the chunk phase the render of p would run, its chunks built as the render builds them
int xrt_test_chunk_plan(xrt_ctx* c, const xrt_render_params* p, uint32_t plan[5], uint32_t* sizes, uint32_t n_sizes) {
    c = first_device(c);
    if (!c || !p || !plan || (!sizes && n_sizes)) return XRT_ERR_INVALID;
    ChunkProbe probe{0, 0, 0, 0, sizes, n_sizes};
    std::memset(plan, 0, 5 * sizeof(uint32_t));
    if ((size_t)shard_rows(p->height, p->shard_index, p->shard_count) * p->width == 0) return check_render(c, p);
    xrt_render_params q = *p;
    q.flags &= ~(uint32_t)XRT_FLAG_ACCUMULATE;   // the context's own framebuffer, cleared
    const int rc = render_impl(c, &q, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &probe);
    if (rc) return rc;
    plan[0] = probe.passes != 0 && probe.blocks != 0, plan[1] = probe.passes, plan[2] = probe.chunks, plan[3] = probe.blocks, plan[4] = probe.cap;
    return XRT_OK;
}

// ---------------------------------------------------------- variance render ----
// xrt_render_var / xrt_render_var_device: render_impl (render_multi) with a variance plane.  The
// plane is rendered into device memory — the context's own for the host entry point — and the
// frame is left in the context's framebuffer, where xrt_tonemap and the filters read it.
static int render_var(xrt_ctx* c, const xrt_render_params* p, float* d_out, float* h_out, float* d_var, float* h_var,
                      xrt_stats* st, int wait, hipStream_t wait_stream) {
    if (!c || !p || !(d_out || h_out) || !(d_var || h_var)) return set_err(c, XRT_ERR_INVALID, "xrt_render_var: null argument");
    xrt_ctx* c0 = first_device(c);
    const size_t npix = (size_t)p->width * p->height;
    int rc;
    if (!d_var) {
        HIPCHK(c, hipSetDevice(c0->device));
        if ((rc = ensure(c0, c0->var, npix * sizeof(float)))) return c0 == c ? rc : multi_fail(c, c0, rc, "variance plane");
        d_var = as<float>(c0->var);
    }
    rc = !c->subs.empty() ? render_multi(c, p, d_out, h_out, st, wait, wait_stream, d_var)
                          : render_impl(c, p, d_out, h_out, st, wait, wait_stream, d_var);
    if (rc) return rc;
    if (h_var) HIPCHK(c, hipMemcpy(h_var, d_var, npix * sizeof(float), hipMemcpyDeviceToHost));
    if (d_out) {   // the caller's image: the context's framebuffer gets a copy
        if ((rc = ensure(c0, c0->fb, npix * 3 * sizeof(float)))) return c0 == c ? rc : multi_fail(c, c0, rc, "framebuffer");
        HIPCHK(c, hipMemcpy(c0->fb.p, d_out, npix * 3 * sizeof(float), hipMemcpyDeviceToDevice));
    }
    return XRT_OK;
}

int xrt_render_var(xrt_ctx* c, const xrt_render_params* p, float* rgb_out, float* variance_out, xrt_stats* st) {
    return render_var(c, p, nullptr, rgb_out, nullptr, variance_out, st, 0, nullptr);
}

int xrt_render_var_device(xrt_ctx* c, const xrt_render_params* p, float* d_rgb_out, float* d_variance_out,
                          void* hip_stream, xrt_stats* st) {
    return render_var(c, p, d_rgb_out, nullptr, d_variance_out, nullptr, st, 2, (hipStream_t)hip_stream);
}

}  // extern "C"
