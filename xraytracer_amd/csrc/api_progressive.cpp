// api_progressive.cpp — the C ABI of include/xrt.h, progressive rendering: a frame rendered in passes
// that add samples (xrt_progressive_*).  A pass is render_impl's sequence (api_render.cpp) with the two
// steps that make a render one-shot taken out: k_seed's reset runs once, in begin, and every add starts
// with k_resume instead; the division is k_progress_frame's, out of place, so the accumulator keeps the
// pixels' running sums (progressive.hip).  Everything between — parameters, plan, lists, chunks, the
// schedules' loops, stats — is render_impl's own pieces.
#include <chrono>
#include <cstring>

#include "ctx.h"

namespace xrt {
namespace {

// The render parameters of a session: the caller's with the flags of the schedules that can be resumed
// (no speculative starts, no pixel-parallel chains: their kernels keep no per-slot stream position a
// later pass could start from).  With the variance option the plan is xrt_render_var's under
// XRT_FLAG_VAR_FUSED, which under XRT_FLAG_WAVEFRONT takes no launch geometry.
xrt_render_params session_params(const xrt_render_params& p, bool variance) {
    xrt_render_params q = p;
    q.flags = (p.flags & ~(uint32_t)XRT_FLAG_VAR_FUSED) | XRT_FLAG_NO_SPEC | XRT_FLAG_NO_PIXEL;
    if (variance && (p.flags & XRT_FLAG_WAVEFRONT)) {
        q.flags = (p.flags & XRT_FLAG_TIMING) | XRT_FLAG_WAVEFRONT | XRT_FLAG_NO_SPEC | XRT_FLAG_NO_PIXEL;
        q.slots_per_wave = q.visits_per_launch = 0;
    }
    return q;
}

// Parameters, plan and lists of a pass of spp samples (begin: of the seeding).  The slot -> pixel map
// and the partitions follow from the shard's size and the flags, so every pass gets the same ones; the
// refill threshold and the chunk phase may differ from pass to pass.  The sums go to the accumulator,
// the kernels are told that the slots' records persist (kRflagSession), and no pixel is retired before
// the path loop: k_camlist would write absolute stream positions and counters.
int session_plan(xrt_ctx* c, uint32_t spp, KParams& P, RenderPlan& R, LiveLists& L) {
    const ProgressiveSession& S = c->prog;
    xrt_render_params q = S.p;
    q.spp = spp;
    P = render_params(c, &q, S.n, as<float>(c->acc));
    P.rflags |= kRflagSession;
    R = plan_render(P, &q, S.variance ? as<float2>(c->mom) : nullptr);
    R.elide = false;
    if (R.rng_keep > kMT) return set_err(c, XRT_ERR_INVALID, "visits_per_launch too large for the RNG ring");
    return bind_plan(c, P, R, L);
}

int begin_session(xrt_ctx* c, const xrt_render_params* p, uint32_t options) {
    int rc = order_after(c, 0, nullptr, false);
    if (rc) return rc;
    ProgressiveSession& S = c->prog;
    S = ProgressiveSession{};
    S.variance = (options & XRT_PROGRESSIVE_VARIANCE) != 0;
    S.p = session_params(*p, S.variance);
    S.n = (size_t)shard_rows(p->height, p->shard_index, p->shard_count) * p->width;
    const size_t npix = (size_t)p->width * p->height;
    if ((rc = ensure(c, c->acc, npix * 3 * sizeof(float)))) return rc;
    HIPCHK(c, hipMemsetAsync(c->acc.p, 0, npix * 3 * sizeof(float), c->stream));
    if (S.n) {
        if ((rc = grow_slots(c, S.n)) || (S.variance && (rc = ensure(c, c->mom, S.n * sizeof(float2))))) return rc;
        if (S.variance) HIPCHK(c, hipMemsetAsync(c->mom.p, 0, S.n * sizeof(float2), c->stream));
        KParams P;
        RenderPlan R;
        LiveLists L{};
        if ((rc = session_plan(c, 1, P, R, L))) return rc;
        xrt_stats unused{};
        LaunchTimer T{c, unused, false, {}, {}};
        if ((rc = seed_paths(c, P, R, L, T))) return rc;   // k_seed and every slot's first twist
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.active = true;
    return XRT_OK;
}

int add_samples(xrt_ctx* c, uint32_t spp, xrt_stats* st) {
    const auto t_start = std::chrono::steady_clock::now();
    int rc = order_after(c, 0, nullptr, false);
    if (rc) return rc;
    ProgressiveSession& PS = c->prog;
    xrt_stats S{};
    S.path_slots = PS.n;
    uint64_t resumed = 0;
    if (PS.n) {
        KParams P;
        RenderPlan R;
        LiveLists L{};
        if ((rc = session_plan(c, spp, P, R, L))) return rc;
        LaunchTimer T{c, S, (PS.p.flags & XRT_FLAG_TIMING) != 0, {}, {}};
        HIPCHK(c, hipMemsetAsync(P.stats, 0, 512, c->stream));
        HIPCHK(c, T.launch(XRT_K_SEED, [&] { return launch_resume(P, L.list[0], L.counts(0), L.counts(1), L.req(0), c->stream); }));
        HIPCHK(c, hipMemcpyAsync(c->kparams.p, &P, sizeof(KParams), hipMemcpyHostToDevice, c->stream));
        ChunkBufs CB{};
        if (R.chunk_passes && (rc = build_chunks(c, P, R, L, T, CB))) return rc;
        uint64_t it = 0;
        bool done = false;
        if ((rc = run_paths(c, P, R, L, CB, T, it, done))) return rc;
        HIPCHK(c, T.launch(XRT_K_FINISH, [&] { return launch_progress_finish(P, c->stream); }));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!done && (rc = check_drained(c, P, R, L, it))) return rc;
        if ((rc = read_stats(c, P, S))) return rc;   // the slots' counters are the session's so far
        unsigned long long word = 0;
        HIPCHK(c, hipMemcpy(&word, P.stats + kStatsResume, sizeof(word), hipMemcpyDeviceToHost));
        resumed = word;
        const uint64_t twists = S.rng_twists;   // every twist of the slots since begin
        S.rng_twists = twists - PS.twists;
        PS.twists = twists;
        plan_stats(P, R, it, S);
        T.read_out();
    }
    PS.spp_done += spp;
    PS.passes++;
    PS.resume_twists = (uint32_t)resumed;
    S.samples = (uint64_t)PS.n * PS.spp_done;
    S.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (st) *st = S;
    return XRT_OK;
}

// the frame of the samples so far into device memory (d_rgb / d_var: the caller's, else the context's
// own) and from there into the host arrays given; the context's framebuffer is the frame either way
int session_frame(xrt_ctx* c, float* d_rgb, float* h_rgb, float* d_var, float* h_var, int wait, hipStream_t wait_stream) {
    if (!c) return XRT_ERR_INVALID;
    const ProgressiveSession& S = c->prog;
    if (!S.active) return set_err(c, XRT_ERR_INVALID, "xrt_progressive_frame: no session is open on the context");
    if (!d_rgb && !h_rgb) return set_err(c, XRT_ERR_INVALID, "xrt_progressive_frame: null output");
    if (S.spp_done == 0) return set_err(c, XRT_ERR_INVALID, "xrt_progressive_frame: no samples yet (xrt_progressive_add first)");
    const bool want_var = d_var || h_var;
    if (want_var && !S.variance)
        return set_err(c, XRT_ERR_INVALID, "xrt_progressive_frame: the session was begun without XRT_PROGRESSIVE_VARIANCE");
    if (want_var && S.spp_done < 2)
        return set_err(c, XRT_ERR_INVALID, "xrt_progressive_frame: a variance needs at least 2 samples (one sample has none)");
    int rc = order_after(c, wait, wait_stream, false);
    if (rc) return rc;
    const size_t npix = (size_t)S.p.width * S.p.height;
    if ((rc = ensure(c, c->fb, npix * 3 * sizeof(float))) || (want_var && !d_var && (rc = ensure(c, c->var, npix * sizeof(float)))))
        return rc;
    float* rgb = d_rgb ? d_rgb : as<float>(c->fb);
    float* var = !want_var ? nullptr : d_var ? d_var : as<float>(c->var);
    HIPCHK(c, hipMemsetAsync(rgb, 0, npix * 3 * sizeof(float), c->stream));   // outside the shard: +0
    if (var) HIPCHK(c, hipMemsetAsync(var, 0, npix * sizeof(float), c->stream));
    if (S.n) {
        xrt_render_params q = S.p;
        q.spp = S.spp_done;
        KParams P = render_params(c, &q, S.n, as<float>(c->acc));
        P.slot_mul = plan_render(P, &q, nullptr).slot_mul;
        HIPCHK(c, launch_progress_frame(P, rgb, as<float2>(c->mom), var, c->stream));
    }
    if (d_rgb) HIPCHK(c, hipMemcpyAsync(c->fb.p, d_rgb, npix * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_rgb) HIPCHK(c, hipMemcpy(h_rgb, rgb, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (h_var) HIPCHK(c, hipMemcpy(h_var, var, npix * sizeof(float), hipMemcpyDeviceToHost));
    return XRT_OK;
}

}  // namespace
}  // namespace xrt

using namespace xrt;

extern "C" {

int xrt_progressive_begin(xrt_ctx* c, const xrt_render_params* p, uint32_t options) {
    if (!c || !p) return XRT_ERR_INVALID;
    if (!c->subs.empty())
        return set_err(c, XRT_ERR_UNSUPPORTED,
                       "xrt_progressive_begin: a multi-device context (run one session per device over row shards)");
    int rc = check_render(c, p);
    if (rc) return rc;
    if (options & ~(uint32_t)XRT_PROGRESSIVE_VARIANCE) return set_err(c, XRT_ERR_INVALID, "xrt_progressive_begin: unknown option");
    if (p->integrator == XRT_INTEGRATOR_WHITTED)
        return set_err(c, XRT_ERR_UNSUPPORTED,
                       "xrt_progressive_begin: WhittedIntegrator (its kernels keep no stream position to continue from)");
    if (p->flags & XRT_FLAG_ACCUMULATE)
        return set_err(c, XRT_ERR_UNSUPPORTED, "xrt_progressive_begin: XRT_FLAG_ACCUMULATE (the session owns its accumulator)");
    end_progressive(c);   // a second begin replaces the open session
    if ((rc = begin_session(c, p, options))) end_progressive(c);
    return rc;
}

int xrt_progressive_add(xrt_ctx* c, uint32_t spp, xrt_stats* st) {
    if (!c) return XRT_ERR_INVALID;
    if (!c->prog.active) return set_err(c, XRT_ERR_INVALID, "xrt_progressive_add: no session is open on the context");
    if (spp == 0) return set_err(c, XRT_ERR_INVALID, "xrt_progressive_add: spp must be positive");
    if (spp > UINT32_MAX - c->prog.spp_done)
        return set_err(c, XRT_ERR_INVALID, "xrt_progressive_add: the session's sample count would overflow");
    const int rc = add_samples(c, spp, st);
    if (rc) end_progressive(c);   // a pass that failed part-way leaves the slots in no state to continue from
    return rc;
}

int xrt_progressive_frame(xrt_ctx* c, float* rgb_out, float* variance_out) {
    return session_frame(c, nullptr, rgb_out, nullptr, variance_out, 0, nullptr);
}

int xrt_progressive_frame_device(xrt_ctx* c, float* d_rgb_out, float* d_variance_out, void* hip_stream) {
    if (c && !d_rgb_out) return set_err(c, XRT_ERR_INVALID, "xrt_progressive_frame_device: null output");
    return session_frame(c, d_rgb_out, nullptr, d_variance_out, nullptr, 2, (hipStream_t)hip_stream);
}

int xrt_progressive_query(const xrt_ctx* c, xrt_progressive_state* out) {
    if (!c || !out) return XRT_ERR_INVALID;
    const ProgressiveSession& S = c->prog;
    std::memset(out, 0, sizeof(*out));
    if (!S.active) return XRT_OK;
    out->active = 1, out->spp_done = S.spp_done, out->passes = S.passes, out->resume_twists = S.resume_twists;
    out->path_slots = S.n;
    return XRT_OK;
}

int xrt_progressive_end(xrt_ctx* c) {
    if (!c) return XRT_ERR_INVALID;
    end_progressive(c);
    return XRT_OK;
}

}  // extern "C"
