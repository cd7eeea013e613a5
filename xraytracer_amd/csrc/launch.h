// launch.h — host-callable kernel launchers and their eligibility / sizing helpers, grouped
// below by the unit (*.hip) that defines them, after what the launchers themselves share: the
// runtime-value-to-template dispatch (with_const, with_scene_kind, with_integrator) and the grid
// of the persistent pixel kernels (persistent_blocks).  The BVH kernels' dispatch on the stack
// entry type is with_stack_entry (bvh_walk.h) and with_whit_bvh (whit_trace.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "slot_map.h"
#include "step_chunks.h"
#include "step_groups.h"
#include "wavefront.h"

namespace xrt {
// Experiment switches (tools/*.sh) are read from the environment only in builds made with
// -DXRT_EXPERIMENTS (csrc/Makefile `variant`); the shipped library never reads them.
#ifdef XRT_EXPERIMENTS
inline const char* exp_env(const char* name) { return std::getenv(name); }
#else
inline const char* exp_env(const char*) { return nullptr; }
#endif
// Runtime value -> template argument, for launchers whose kernels are instantiated per scene
// kind, integrator or light count: calls fn(std::integral_constant<int, V>{}) for the first listed V that
// equals v (the last one when none does) and returns what fn returns.  fn is a generic lambda
// that uses its argument as a constant expression (`k_shade<SCN, I>`); a build that exists for
// some values only is an `if constexpr (I == ...)` inside it, so exactly the kernels the
// lambda names for the listed values are instantiated.
template <int V, int... Rest, typename F>
auto with_const(int v, F&& fn) {
    if constexpr (sizeof...(Rest) == 0) {
        return fn(std::integral_constant<int, V>{});
    } else {
        if (v == V) return fn(std::integral_constant<int, V>{});
        return with_const<Rest...>(v, fn);
    }
}
template <typename F>
auto with_scene_kind(int kind, F&& fn) {
    return with_const<SCN_TRI, SCN_SPHERE, SCN_MIXED>(kind, fn);
}
template <typename F>
auto with_integrator(int integrator, F&& fn) {
    return with_const<XRT_INTEGRATOR_DIRECT, XRT_INTEGRATOR_VPT, XRT_INTEGRATOR_INDIRECT, XRT_INTEGRATOR_NORMAL,
                      XRT_INTEGRATOR_VPT_NEE, XRT_INTEGRATOR_GI>(integrator, fn);
}
// Grid of a persistent kernel that takes the shard's n_slots pixels from a counter, one wave per
// pixel at a time: as many blocks as fit on the device at once (the occupancy of `kernel` at
// `block` threads and `lds` dynamic LDS bytes, times the CUs), at most one wave per pixel, at
// least one block.
template <typename K>
hipError_t persistent_blocks(K kernel, int block, size_t lds, uint32_t n_slots, uint32_t* blocks) {
    int dev = 0, ncu = 0, per_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds);
    if (e != hipSuccess) return e;
    const uint64_t want = ((uint64_t)n_slots + block / 64 - 1) / (block / 64);
    *blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, per_cu) * ncu, want));
    return hipSuccess;
}

// ---------------------------------------------------------------------- frame.hip ----
hipError_t launch_seed(const KParams& P, uint32_t* list, uint32_t* count, uint32_t* count_other,
                       uint32_t* req_count, hipStream_t st);
hipError_t launch_finish(const KParams& P, hipStream_t st);
// a variance render's plane: the slots' {s1, s2} records (k_shade / k_whitted with a `mom`) into
// var [height][width], the shard's pixels only (xrt_render_var's last five operations)
hipError_t launch_finish_var(const KParams& P, const float2* mom, float* var, hipStream_t st);
// out[s] = col + width * row of slot s under P's slot -> pixel map (xrt_test_slot_map)
hipError_t launch_test_slot_map(const KParams& P, uint32_t* out, hipStream_t st);
// Image::gammaCorrection + writePPM quantisation of n floats into n bytes
hipError_t launch_tonemap(const float* rgb, uint32_t n, float inv_gamma, uint8_t* out, hipStream_t st);

// ---------------------------------------------------------------- progressive.hip ----
// A progressive session's pass (xrt_progressive_add) between launch_resume and launch_progress_finish.
// launch_resume takes launch_seed's arguments and leaves its lists and counters (nothing requested),
// but of a slot only restarts the sample loop: streams, counters and moments stay, and a ring with fewer
// than P.rng_keep words ahead is twisted (counted in stats[kStatsResume])
hipError_t launch_resume(const KParams& P, uint32_t* list, uint32_t* count, uint32_t* count_other, uint32_t* req_count,
                         hipStream_t st);
hipError_t launch_progress_finish(const KParams& P, hipStream_t st);   // launch_finish's counters, no division
// rgb [height][width][3] = P.fb / P.spp and, with mom and var, var [height][width] as launch_finish_var's,
// the shard's pixels only
hipError_t launch_progress_frame(const KParams& P, float* rgb, const float2* mom, float* var, hipStream_t st);

// ---------------------------------------------------------------------- trace.hip ----
// zero_deep: clear the two-level trace's queue counters first (false when the k_shade that
// precedes this trace in the render loop has cleared them)
hipError_t launch_trace(const KParams& P, const uint32_t* list, const uint32_t* count, uint32_t* zero,
                        uint32_t blocks, hipStream_t st, bool zero_deep = true);
// phase B of a two-level trace (the BVH walk of the rays launch_trace queued); no-op otherwise
hipError_t launch_trace_deep(const KParams& P, hipStream_t st);
// Scene::intersect / occluded for n = P.n_slots caller rays (xrt_query): rays [n][6] on the
// device, tmax [n] or null; list / count (one partition) / zero are scratch
hipError_t launch_query(const KParams& P, const float* rays, const float* tmax, int mode, uint32_t* list,
                        uint32_t* count, uint32_t* zero, xrt_hit* out, hipStream_t st);

// ---------------------------------------------------------------------- shade.hip ----
// mom: a variance render's per-slot {s1, s2} records (n_slots of them; the moments build of
// k_shade), null for a plain render
hipError_t launch_shade(const KParams& P, const uint32_t* list, const uint32_t* count, uint32_t* out,
                        uint32_t* out_count, uint32_t* req_count, uint32_t blocks, hipStream_t st, float2* mom = nullptr);

// ----------------------------------------------------------------------- step.hip ----
// fused schedule (k_step): LDS bytes it needs for this scene, 0 = scene too large for it
size_t step_lds_bytes(const KParams& P);
bool use_step_tri(const KParams& P);   // triangle scene: k_step_tri (cooperative traces)
// up to `visits` path segments per live slot; appends survivors to out (partitioned
// counters out_count); twists the rings of slots that ran low in-line; clears zero
// (next-next round).  req_count is unused by the step kernels (kept in the signature of
// every schedule's step launch; only the seeding k_refill reads the request list)
// dP: device copy of P (the triangle-scene kernel reads its parameters from memory)
// tri: the caller's use_step_tri(P), decided once per render (k_step_tri instead of k_step)
// mom: as launch_shade's (the moments builds of k_step / k_step_tri, XRT_FLAG_VAR_FUSED)
hipError_t launch_step(const KParams& P, const KParams* dP, const uint32_t* list, const uint32_t* count, uint32_t* out,
                       uint32_t* out_count, uint32_t* zero, uint32_t* req_count, uint32_t visits, uint32_t blocks,
                       uint64_t live, bool tri, hipStream_t st, float2* mom = nullptr);

// --------------------------------------------------------------------- refill.hip ----
// twist the rings of the slots on P.req (count at *count); clears *zero_count
hipError_t launch_refill(const KParams& P, const uint32_t* count, uint32_t* zero_count, hipStream_t st);
// the merged schedule's refill (leaves ST_RNGREQ to the merged kernel; see refill.hip)
hipError_t launch_refill_merged(const KParams& P, const uint32_t* count, uint32_t* zero_count, hipStream_t st);

// ---------------------------------------------------------------- step_merged.hip ----
// merged-trace triangle schedule (the kernels: step_merged.h): eligibility, RNG words one segment may
// draw, LDS bytes, and the launch (same list / counter contract as launch_step; SO: the
// kernel-argument object records, build_step_objs in wavefront.h)
bool use_step_merged(const KParams& P);
bool use_step_bvh(const KParams& P);     // two-level scenes: the merged kernel with the wave's BVH walk
uint32_t step_merged_draws(const KParams& P);
uint32_t step_merged_spw(const KParams& P, uint64_t live);   // slots per wave for `live` live slots
uint32_t step_merged_group(const KParams& P, uint32_t spw);  // lanes per slot in group traces (1 = none)
size_t step_merged_lds_bytes(const KParams& P);
// groups, group: the launch serves the partitions of group `group` of `groups` only (step_groups.h:
// their lists, their counters in out_count and zero); 1, 0: every partition.  live and
// live_part_max are the whole shard's either way
// mom: as launch_shade's (the moments builds, a unit of their own: step_merged_mom.hip)
hipError_t launch_step_merged(const KParams& P, const KParams* dP, const StepObjs& SO, const uint32_t* list,
                              const uint32_t* count, uint32_t* out, uint32_t* out_count, uint32_t* zero,
                              uint32_t* req_count, uint32_t visits, uint64_t live, uint32_t live_part_max,
                              uint32_t groups, uint32_t group, hipStream_t st, float2* mom = nullptr);
// The whole-wave phase in block-owned chunks (step_chunks.h).  The chunk buffer: header words (chunks
// and live slots per class), the partitions' live counts without the retired pixels, two counters
// per chunk and two segments of kChunkSlots entries per chunk, for 8 * class_cap chunks.
struct ChunkBufs {
    uint32_t *hdr, *part_live, *cnt, *seg;
    uint32_t class_cap;
    uint32_t chunks, blocks;   // after the build: chunks that hold a slot; blocks of a launch of the phase (0: the phase does not run)
};
// one launch of the phase, numbered rot: `passes` passes of `visits` visits per block; adds the live
// slots left to live_count (n_part words, cleared before) and clears zero, as a step launch does
hipError_t launch_step_merged_chunks(const KParams& P, const KParams* dP, const StepObjs& SO, const ChunkBufs& B,
                                     uint32_t* live_count, uint32_t* zero, uint32_t visits, uint32_t passes, uint32_t rot,
                                     hipStream_t st);
#if XRT_PHASE_CLOCK
// experiment builds: the merged kernels' per-wave entry / exit clocks of the work queued on st so far,
// written to `path` (null: dropped) and cleared; tools/wave_timeline.py reads the file
hipError_t wave_clock_dump(const char* path, hipStream_t st);
#endif

// ---------------------------------------------------------------- chunk_lists.hip ----
// the chunks from the seeded partition lists (header and counters cleared by the caller before)
hipError_t launch_chunks_build(const KParams& P, const ChunkBufs& B, const uint32_t* list, const uint32_t* count,
                               hipStream_t st);
// the chunks' live slots onto the partition lists `out` (counters out_count, cleared before)
hipError_t launch_chunks_scatter(const KParams& P, const ChunkBufs& B, uint32_t* out, uint32_t* out_count, hipStream_t st);

// ----------------------------------------------------------------------- spec.hip ----
// speculative sample starts for the merged schedule's group layouts: eligibility,
// the per-slot camera lists (once per render, before the first speculative launch; with
// `retire`, right after the seeding refill, and the pixels whose list is empty are finished
// there: it then runs whether or not P.camlist is set), and the step launch at spw = 16, 8 or
// 4 slots per wave (same list / counter contract as launch_step_merged)
bool use_step_spec(const KParams& P);
constexpr uint32_t kSpecDraws = 11;   // stream words one k_step_spec visit may read past the cursor
hipError_t launch_camlist(const KParams& P, bool retire, hipStream_t st);
hipError_t launch_step_spec(const KParams& P, const KParams* dP, const uint32_t* list, const uint32_t* count,
                            uint32_t* out, uint32_t* out_count, uint32_t* zero, uint32_t visits, uint32_t part_live,
                            uint32_t spw, hipStream_t st);

// ---------------------------------------------------------------------- pixel.hip ----
// pixel-parallel sample chains (pixel.hip): Direct / Normal scenes that fit the LDS scene
// carve; one launch renders every pixel of the shard (after k_seed, before k_finish), taking
// pixels from the counter at `work` (zeroed by the launcher)
bool use_pixel(const KParams& P);
size_t pix_lds_bytes(const KParams& P);
hipError_t launch_pixel(const KParams& P, uint32_t* work, hipStream_t st);

// -------------------------------------------------------------------- whitted.hip ----
// WhittedIntegrator (whitted.hip): scenes that fit the LDS scene carve; one launch renders
// every pixel of the shard, with launch_pixel's contract (after k_seed, before k_finish, the
// pixel counter at `work`)
bool use_whitted(const KParams& P);
size_t whit_lds_bytes(const KParams& P);
// mom: as launch_shade's
hipError_t launch_whitted(const KParams& P, uint32_t* work, hipStream_t st, float2* mom = nullptr);
// ... and triangle scenes beyond it that have the triangle BVH (one- and two-level scenes):
// k_whitted_bvh, the same loop tracing through the BVH and the small objects' LDS copy
// (XRT_FLAG_WHITTED_BVH; same contract)
bool use_whitted_bvh(const KParams& P);
size_t whit_bvh_lds_bytes(const KParams& P);
hipError_t launch_whitted_bvh(const KParams& P, uint32_t* work, hipStream_t st, float2* mom = nullptr);
// k_whitted's reflect / refract / fresnel / normalize over n inputs {I, N}: 13 floats each
hipError_t launch_test_whitted(const float* in, uint32_t n, float* out, hipStream_t st);

// ------------------------------------------------------------------------ aov.hip ----
// First-hit guide buffers (aov.hip, xrt_render_aov): the planes k_aov / k_aov_bvh write for the
// shard's pixels (device pointers; null = not wanted) and the per-object raw albedo table
// xrt_upload_scene leaves (3 floats per object).  aov_kernel: 1 = k_aov (the scene fits the
// LDS carve, use_whitted), 2 = k_aov_bvh (a triangle scene with the BVH, use_whitted_bvh),
// 0 = neither holds the scene.  launch_aov has launch_pixel's contract (after k_seed; the
// pixel counter at `work`) but divides and writes its planes itself: no k_finish.
struct AovOut {
    float *albedo, *normal, *depth, *alpha;
    int32_t* object;
    const float* obj_albedo;
};
int aov_kernel(const KParams& P);
hipError_t launch_aov(const KParams& P, const AovOut& A, uint32_t* work, hipStream_t st);

// -------------------------------------------------------------------- denoise.hip ----
// The two a-trous filters (denoise.hip): the edge-avoiding one (xrt_denoise) and the variance-guided
// one (xrt_denoise_var), which share records, kernels and launches.  launch_denoise_pack gathers the
// caller's planes (device pointers; color is required, a null plane packs as zeros) into the
// per-pixel records col = {c.rgb, variance}, nrm = {n.xyz, object bits}, alb = {albedo.rgb, depth};
// the plain filter passes no variance and carries +0 there.  launch_dnv_estimate (the variance
// filter without a caller's variance) reads cin's rgb and nrm's object and writes cout = {cin.rgb,
// the estimated variance}: cout is another buffer than cin, so no lane reads what the launch writes.
// launch_denoise_iter runs one iteration of `filter` with tap spacing `step` pixels from cin: into
// the col records cout, or, when out3 is set (the last iteration), into that packed float3 image
// and, when outv is set (the variance filter only), that variance plane.  tiled: through the
// LDS-tiled kernel, which exists for the steps denoise_has_tiled names; both kernels give the same
// bits.
enum class DenoiseFilter { Plain, Var };
struct DenoiseK {
    // k0: the plain filter's factor on the squared colour distance; the variance filter's
    // sigma_luminance (<= 0: off).  The factors on the squared normal / depth / albedo distance.
    float k0, kn, kz, ka;
};
struct DenoiseIter {
    const f4 *cin, *nrm, *alb;
    f4* cout;
    float *out3, *outv;
    uint32_t width, height;
    int step;
    DenoiseK K;
};
hipError_t launch_denoise_pack(const float* color, const float* variance, const float* albedo, const float* normal,
                               const float* depth, const int32_t* object, size_t npix, f4* col, f4* nrm, f4* alb,
                               hipStream_t st);
hipError_t launch_dnv_estimate(const f4* cin, const f4* nrm, f4* cout, uint32_t width, uint32_t height, int radius,
                               hipStream_t st);
bool denoise_has_tiled(int step);
hipError_t launch_denoise_iter(DenoiseFilter filter, const DenoiseIter& I, bool tiled, hipStream_t st);
// pixels per block of every filter kernel: a wave is two 32-pixel row pieces
constexpr int kDnTileW = 32, kDnTileH = 8;
constexpr int kDnBlock = kDnTileW * kDnTileH;

// ------------------------------------------------------------------- selftest.hip ----
hipError_t launch_test_rng(const uint32_t* seeds, uint32_t n_seeds, uint32_t skip, uint32_t n, float* out,
                           uint32_t* rings, hipStream_t st);
hipError_t launch_test_trig(const float* x, uint32_t n, float* out, hipStream_t st);
hipError_t launch_test_trig_domain(uint32_t first, uint32_t count, float* s, float* c, float* r, hipStream_t st);
hipError_t launch_test_logexp(const float* x, uint32_t n, float* out, hipStream_t st);
hipError_t launch_test_powf(const float* x, uint32_t n, float y, float* out, hipStream_t st);
hipError_t launch_test_fastdiv(uint32_t mode, float c, float rc, uint32_t first, uint32_t count,
                               unsigned long long* nbad, uint32_t* bad, hipStream_t st);
// medium.h's medium_density of M at n points {x, y, z}
hipError_t launch_test_density(const DMedium& M, const float* pts, uint32_t n, float* out, hipStream_t st);
// medium.h's hg_sample / sample_wavelength over n items; item i draws from its own eight raw
// stream words words[8 i ..], cursor 0
hipError_t launch_test_hg(float g, const float* wo, const uint32_t* words, uint32_t n, float* wi, hipStream_t st);
hipError_t launch_test_wavelength(const float* thr, const float* albedo, const uint32_t* words, uint32_t n,
                                  uint32_t* channel, float* pmf, hipStream_t st);
}  // namespace xrt
