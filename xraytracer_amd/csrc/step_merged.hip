// step_merged.hip — the plain builds of the merged step kernels (step_merged.h): their launches, the
// chunk phase's step launch, the host-side eligibility and layout rules of the schedule, and the
// experiment builds' wave clock dump.  The moments builds are step_merged_mom.hip.
#include <cstdio>
#include <vector>

#include "step_merged.h"

namespace xrt {

#if XRT_PHASE_CLOCK
hipError_t wave_clock_dump(const char* path, hipStream_t st) {
    unsigned int n = 0, m = 0, zero = 0;
    int khz = 0, dev = 0;
    hipError_t e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_wave_clock_n), sizeof(n));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_wave_clock_n), &zero, sizeof(zero));
    if (e == hipSuccess) e = hipMemcpyFromSymbol(&m, HIP_SYMBOL(g_pass_clock_n), sizeof(m));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_pass_clock_n), &zero, sizeof(zero));
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
    if (e != hipSuccess || !path) return e;
    n = std::min(n, kWaveClockCap);
    std::vector<WaveClockRec> rec(n);
    if (n) e = hipMemcpyFromSymbol(rec.data(), HIP_SYMBOL(g_wave_clock), (size_t)n * sizeof(WaveClockRec));
    m = std::min(m, kPassClockCap);
    std::vector<PassClockRec> pass(m);   // the chunk kernel's pass ends (step_sources.h)
    if (m && e == hipSuccess) e = hipMemcpyFromSymbol(pass.data(), HIP_SYMBOL(g_pass_clock), (size_t)m * sizeof(PassClockRec));
    if (e != hipSuccess) return e;
    if (FILE* f = std::fopen(path, "wb")) {   // header: record count, wall clock kHz; then the records; then the pass ends likewise
        const uint32_t head[2] = {n, (uint32_t)khz};
        std::fwrite(head, sizeof(head), 1, f);
        std::fwrite(rec.data(), sizeof(WaveClockRec), n, f);
        std::fwrite(&m, sizeof(m), 1, f);
        std::fwrite(pass.data(), sizeof(PassClockRec), m, f);
        std::fclose(f);
    }
    return hipSuccess;
}
#endif

hipError_t launch_step_merged(const KParams& P, const KParams* dP, const StepObjs& SO, const uint32_t* list,
                              const uint32_t* count, uint32_t* out, uint32_t* out_count, uint32_t* zero,
                              uint32_t* req_count, uint32_t visits, uint64_t live, uint32_t live_part_max,
                              uint32_t groups, uint32_t group, hipStream_t st, float2* mom) {
    if (mom)
        return launch_step_merged_mom(P, dP, SO, list, count, out, out_count, zero, mom, visits, live, live_part_max, groups,
                                      group, st);
    return launch_step_merged_as<false>(P, dP, SO, list, count, out, out_count, zero, req_count, visits, live, live_part_max,
                                        groups, group, st);
}

hipError_t launch_step_merged_chunks(const KParams& P, const KParams* dP, const StepObjs& SO, const ChunkBufs& B,
                                     uint32_t* live_count, uint32_t* zero, uint32_t visits, uint32_t passes, uint32_t rot,
                                     hipStream_t st) {
    if (P.two_level || visits == 0 || visits > 255u || passes == 0 || passes > 255u || B.blocks == 0 ||
        B.blocks % 8u || B.blocks > 8u * kChunkClassBlocks)
        return hipErrorInvalidValue;
    const uint32_t blocks = B.blocks;   // from the chunks as built: 8 per chunk of the fullest class (build_chunks)
    const size_t lds = step_merged_lds_bytes(P);
    with_const<XRT_INTEGRATOR_DIRECT, XRT_INTEGRATOR_GI>(P.integrator, [&](auto integ) {   // use_step_merged
        with_const<0, 1, 2, 3, 4>(P.n_lights, [&](auto nl) {
            hipLaunchKernelGGL((k_step_merged_chunks<decltype(integ)::value, decltype(nl)::value>), dim3(blocks), dim3(kBlock),
                               lds, st, dP, SO, B.hdr, B.cnt, B.seg, live_count, zero, visits, passes, rot);
        });
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------- host side ----
bool use_step_merged(const KParams& P) {
    return P.scene_kind == SCN_TRI && P.small_tri && P.det_bounded && P.n_objs <= kMergedMaxObjs && P.n_lights <= kMaxLights &&
           (P.integrator == XRT_INTEGRATOR_DIRECT || (P.integrator == XRT_INTEGRATOR_GI && P.max_depth > 0)) &&
           !exp_env("XRT_NO_MERGED") && step_merged_lds_bytes(P) <= kStepLds;
}

// The merged schedule for two-level scenes (C4): k_step_merged<..., BVH = true>.  The small
// objects must be traceable by pair passes (KParams::sstep: at most kMergedMaxObjs objects,
// det_bounded), the 4-wide BVH's node indices fit the 16-bit quad stacks, one or two area
// lights (the kernel's two pair-pass scratch buffers per wave must fit kStepLds).
bool use_step_bvh(const KParams& P) {
    return P.scene_kind == SCN_TRI && P.two_level && P.sstep && P.det_bounded && P.bvh4 && P.bvh_node &&
           P.bvh4_nodes <= 0x10000 && P.bvh4_stack > 0 && P.bvh4_stack <= kBvh4Stack && P.n_lights >= 1 &&
           P.n_lights <= 2 &&
           (P.integrator == XRT_INTEGRATOR_DIRECT || (P.integrator == XRT_INTEGRATOR_GI && P.max_depth > 0)) &&
           !exp_env("XRT_NO_STEP_BVH") && step_merged_lds_bytes(P) <= kStepLds;
}

uint32_t step_merged_draws(const KParams& P) { return 6u + 2u * (uint32_t)P.n_lights; }

static size_t merged_wave_bytes(int n_lights) {
    return with_const<0, 1, 2, 3, 4>(n_lights, [](auto nl) { return sizeof(MergedWave<decltype(nl)::value>); });
}

size_t step_merged_lds_bytes(const KParams& P) {
    const size_t w = merged_wave_bytes(P.n_lights);
    if (P.two_level) return bvh_step_layout(P, (uint32_t)w).total;
    return merged_wave_off(P, step_layout(P)) + (kBlock / 64) * w;
}

// slots per wave for a shard of `live` slots
// (xrt_render_params.slots_per_wave overrides it; results do not depend on it)
uint32_t step_merged_spw(const KParams& P, uint64_t live) {
    const bool group = P.n_tris <= 64 && !(P.rflags & XRT_FLAG_NO_GROUP);   // 4 slots per wave: group traces only
    if (P.spw_req == 4) return group ? 4u : 16u;
    if (P.spw_req == 8) return group ? 8u : 16u;
    if (P.spw_req == 16 || P.spw_req == 32 || P.spw_req == 64) return P.spw_req;
    // two-level scenes (C4, tools/spw_sweep.sh): fewer slots per wave leave more
    // quads per deep ray and more lanes per pair pass, which pays once the GPU is not full:
    // full waves above kBvhLive64 live slots, 32 above kBvhLive32, then 16
    if (P.two_level) return live >= kBvhLive64 ? 64u : live >= kBvhLive32 ? 32u : 16u;
    // measured on C2 (tools/shard_sim.py): full waves down to ~160k live
    // slots, 32 slots per wave down to ~90k, 16 (4 lanes per slot) down to kMergedLive16,
    // then 4 (16 lanes per slot: the tail of a small shard, where a visit's latency, not
    // issue, sets the time)
    if (live >= kMergedLive64) return 64;
    if (live >= kMergedLive32) return 32;
    if (!group) return 16u;
    if (live < kMergedLive16) return 4u;
    return live < XRT_LIVE8 ? 8u : 16u;
}

// lanes that share one slot's traces at `spw` slots per wave (1 = pair passes over the wave)
uint32_t step_merged_group(const KParams& P, uint32_t spw) {
    const bool group = P.n_tris <= 64 && !(P.rflags & XRT_FLAG_NO_GROUP);   // group trace: 64-bit triangle masks
    return spw < 64 && group ? 64u / spw : 1u;
}

}  // namespace xrt
