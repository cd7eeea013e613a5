// tests/cpp/step_chunks_kat.cpp — checks the block-owned chunks of the merged schedule's whole-wave
// phase (xraytracer_amd/csrc/step_chunks.h, host/step_chunks.cpp) on their own:
// tests/test_step_chunks.py compiles the two files together, plainly and with
// -fsanitize=address,undefined, and runs the program.
//   * Ownership, for C chunks numbered densely, C in {1, 7, 8, 9, 1023, 1024, 1025, 1100, 2049}, and
//     every rot in 0 .. nb / 8: the launch has nb = chunk_blocks(C) = 8 * chunk_class_blocks(fullest
//     class) blocks; every chunk has exactly one owning block, which the block's own enumeration
//     (chunk_owned, chunk_owned_at) names too; c % 8 == b % 8; a block owns floor(C / nb) or
//     ceil(C / nb) chunks, and never more than kChunkOwnMax.
//   * Rotation: where nb < C < 2 nb (1025, 1100), over nb / 8 consecutive launches every chunk is at
//     least once the only chunk of its block, from any first rot.
//   * Dense arrays: chunk_dense_offset and chunk_class_live against a plain concatenation of the
//     partitions' live entries class by class, for partition counts with empty classes (1, 3, 8, 20,
//     256) and partitions without a live entry; chunks_for cuts them.
//   * The passes per launch: chunk_passes' quarter rule, and chunk_plan switching the phase off below
//     two passes and below the whole XRT_CHUNK_PASSES (4 here), without interleaving, with
//     visits_per_launch or slots_per_wave set, when forbidden, for other schedules and for renders beyond a block's table; the force flag.
//   * The rule leaves every parameter set of tests/test_gpu_step_groups.py and
//     tests/test_gpu_interleave.py off chunks (they pin the grouped schedule), and takes the 800 x 600,
//     1024 spp flagship with 4 passes.
// Prints "ok" and returns 0, or the first failure and 1.
#include <cstdio>
#include <vector>

#include "step_chunks.h"

using namespace xrt;

static int fail(const char* what, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    std::printf("FAIL %s (%u, %u, %u, %u)\n", what, a, b, c, d);
    return 1;
}

struct Classes {
    uint32_t nx[8], max_nx, m, nb;
};
static Classes classes_of(uint32_t C) {
    Classes K{};
    for (uint32_t x = 0; x < 8; ++x) {
        K.nx[x] = chunk_class_count(C, x);
        if (K.nx[x] > K.max_nx) K.max_nx = K.nx[x];
    }
    K.m = chunk_class_blocks(K.max_nx);
    K.nb = 8 * K.m;
    return K;
}

// the chunks each block owns in launch rot, by both directions of the map; -1 on a failure
static int owners(uint32_t C, const Classes& K, uint32_t rot, std::vector<uint32_t>& owner, std::vector<uint32_t>& load) {
    owner.assign(C, ~0u);
    load.assign(K.nb, 0);
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t x = c % 8, j = c / 8;
        const uint32_t b = chunk_owner(j, x, K.nx[x], K.m, rot);
        if (b >= K.nb) return fail("owner out of range", C, rot, c, b), -1;
        if (b % 8 != c % 8) return fail("XCD residue", C, rot, c, b), -1;
        owner[c] = b;
        ++load[b];
    }
    std::vector<int> seen(C, 0);
    for (uint32_t b = 0; b < K.nb; ++b) {
        const uint32_t x = b % 8, bj = b / 8, T = K.nx[x] ? chunk_owned(bj, K.nx[x], K.m) : 0;
        if (T != load[b]) return fail("owned count", C, rot, b, T), -1;
        if (T > kChunkOwnMax) return fail("more than the block's table", C, rot, b, T), -1;
        for (uint32_t t = 0; t < T; ++t) {
            const uint32_t j = chunk_owned_at(bj, t, K.nx[x], K.m, rot), c = 8 * j + x;
            if (j >= K.nx[x] || c >= C) return fail("owned chunk out of range", C, rot, b, c), -1;
            if (owner[c] != b) return fail("the two directions disagree", C, rot, b, c), -1;
            if (seen[c]++) return fail("chunk owned twice", C, rot, b, c), -1;
        }
    }
    for (uint32_t c = 0; c < C; ++c)
        if (seen[c] != 1) return fail("chunk without an owner", C, rot, c, (uint32_t)seen[c]), -1;
    return 0;
}

static int check_ownership(uint32_t C) {
    const Classes K = classes_of(C);
    if (K.nb != chunk_blocks(C)) return fail("blocks of a launch", C, K.nb, chunk_blocks(C), 0);
    if (K.nb % 8 || K.nb > 1024 || K.nb == 0) return fail("grid", C, K.nb, 0, 0);
    const uint32_t lo = C / K.nb, hi = (C + K.nb - 1) / K.nb;
    std::vector<uint32_t> owner, load;
    for (uint32_t rot = 0; rot <= K.nb / 8; ++rot) {
        if (owners(C, K, rot, owner, load)) return 1;
        for (uint32_t b = 0; b < K.nb; ++b)
            if (load[b] != lo && load[b] != hi) return fail("share of a block", C, rot, b, load[b]);
    }
    if (C > K.nb && C < 2 * K.nb) {
        const uint32_t starts[] = {0, 5, 1000003};
        for (uint32_t r0 : starts) {
            std::vector<char> single(C, 0);
            for (uint32_t k = 0; k < K.nb / 8; ++k) {
                if (owners(C, K, r0 + k, owner, load)) return 1;
                for (uint32_t c = 0; c < C; ++c)
                    if (load[owner[c]] == 1) single[c] = 1;
            }
            for (uint32_t c = 0; c < C; ++c)
                if (!single[c]) return fail("never singly owned", C, r0, c, 0);
        }
    }
    return 0;
}

static int check_dense(uint32_t n_part, uint32_t seed) {
    std::vector<uint32_t> live(n_part);
    uint32_t s = seed;
    for (uint32_t p = 0; p < n_part; ++p) {
        s = s * 1664525u + 1013904223u;
        live[p] = (s >> 28) == 0 ? 0u : (s >> 8) % 2049u;   // some partitions hold nothing
    }
    for (uint32_t x = 0; x < 8; ++x) {
        uint32_t at = 0;
        for (uint32_t p = x; p < n_part; p += 8) {
            if (chunk_dense_offset(live.data(), p) != at) return fail("dense offset", n_part, p, at, 0);
            at += live[p];
        }
        if (chunk_class_live(live.data(), n_part, x) != at) return fail("class total", n_part, x, at, 0);
        if (x >= n_part && at != 0) return fail("empty class", n_part, x, at, 0);
        const uint32_t nx = chunks_for(at);
        if ((uint64_t)nx * kChunkSlots < at || (nx && (uint64_t)(nx - 1) * kChunkSlots >= at)) return fail("chunks_for", at, nx, 0, 0);
    }
    return 0;
}

// a GPU test's render as the rule sees it: the Cornell box (max_depth 3) at 64 visits per launch unless set
static ChunkRule rule_for(uint32_t slots, uint32_t spp, uint32_t visits_req, uint32_t spw_req, uint32_t flags_force_forbid = 0) {
    ChunkRule r{};
    r.one_level_merged = true;
    r.starts_whole_waves = spw_req == 64 || (spw_req == 0 && slots >= 160000);
    r.interleaved = slots >= 60000;
    r.force = flags_force_forbid & 1, r.forbid = (flags_force_forbid & 2) != 0;
    r.visits_req = visits_req, r.spw_req = spw_req;
    r.spp = spp, r.max_depth = 3, r.visits = visits_req ? visits_req : 64;
    const uint32_t n_part = slots / 2048 ? (slots / 2048 > 256 ? 256 : (slots / 2048 >= 8 ? slots / 2048 & ~7u : slots / 2048)) : 1;
    r.class_cap = chunk_class_cap(n_part, (slots + n_part - 1) / n_part);
    r.pass_cap = 4;
    return r;
}

static int check_rule() {
    if (chunk_passes(8, 1024, 3, 64) != 8 || chunk_passes(16, 1024, 3, 64) != 10 || chunk_passes(8, 256, 3, 64) != 2 ||
        chunk_passes(8, 128, 3, 64) != 1 || chunk_passes(8, 64, 3, 64) != 0 || chunk_passes(8, 4, 3, 0) != 0)
        return fail("chunk_passes", 0, 0, 0, 0);
    if (chunk_plan(rule_for(480000, 1024, 0, 0)) != 4) return fail("the flagship takes 4 passes", 0, 0, 0, 0);
    if (chunk_plan(rule_for(480000, 256, 0, 0)) != 0) return fail("fewer passes than XRT_CHUNK_PASSES", 0, 0, 0, 0);
    if (chunk_plan(rule_for(480000, 410, 0, 0)) != 4 || chunk_plan(rule_for(480000, 409, 0, 0)) != 0)
        return fail("the smallest spp that takes the phase", 0, 0, 0, 0);
    if (chunk_plan(rule_for(480000, 128, 0, 0)) != 0) return fail("below two passes", 0, 0, 0, 0);
    if (chunk_plan(rule_for(480000, 1024, 0, 0, 2)) != 0 || chunk_plan(rule_for(480000, 1024, 0, 0, 3)) != 0)
        return fail("forbidden", 0, 0, 0, 0);
    if (chunk_plan(rule_for(480000, 1024, 64, 0)) != 0 || chunk_plan(rule_for(480000, 1024, 0, 64)) != 0)
        return fail("the caller's launch geometry", 0, 0, 0, 0);
    if (chunk_plan(rule_for(60000, 1024, 0, 0)) != 0) return fail("a shard that starts below whole waves", 0, 0, 0, 0);
    if (chunk_plan(rule_for(432, 6, 3, 64, 1)) != 4 || chunk_plan(rule_for(432, 6, 3, 16, 1)) != 0)
        return fail("forced: whole waves only", 0, 0, 0, 0);
    ChunkRule r = rule_for(480000, 1024, 0, 0);
    r.interleaved = false;
    if (chunk_plan(r) != 0) return fail("row-major renders", 0, 0, 0, 0);
    r = rule_for(480000, 1024, 0, 0, 1);
    r.one_level_merged = false;
    if (chunk_plan(r) != 0) return fail("other schedules", 0, 0, 0, 0);
    r = rule_for(480000, 1024, 0, 0, 1);
    r.class_cap = kChunkOwnMax * kChunkClassBlocks + 1;
    if (chunk_plan(r) != 0) return fail("beyond a block's table", 0, 0, 0, 0);
    // {slots, spp, visits_per_launch, slots_per_wave}: tests/test_gpu_step_groups.py, then tests/test_gpu_interleave.py
    const uint32_t pinned[][4] = {
        {256 * 128, 16, 4, 64}, {384 * 128, 16, 4, 64}, {256 * 128, 48, 4, 64}, {240 * 128, 16, 4, 64}, {640 * 480, 4, 2, 0},
        {256 * 128, 16, 4, 64}, {256 * 128, 2, 2, 64},  {256 * 128, 6, 4, 64},  {256 * 128, 4, 4, 64},
        {64 * 48, 8, 4, 64},    {37 * 29, 8, 4, 64},    {1201, 4, 4, 64},       {64 * 64, 4, 4, 64},     {64 * 12, 4, 4, 64},
        {64 * 48, 4, 4, 64},    {40 * 30, 9, 0, 16},    {40 * 30, 9, 0, 4},     {96 * 64, 2, 2, 64},     {640 * 480, 4, 2, 0}};
    for (const auto& q : pinned)
        if (chunk_plan(rule_for(q[0], q[1], q[2], q[3])) != 0) return fail("a pinned render takes chunks", q[0], q[1], q[2], q[3]);
    return 0;
}

int main() {
    const uint32_t Cs[] = {1, 7, 8, 9, 1023, 1024, 1025, 1100, 2049};
    for (uint32_t C : Cs)
        if (check_ownership(C)) return 1;
    const uint32_t parts[] = {1, 3, 8, 20, 256};
    for (uint32_t n_part : parts)
        for (uint32_t seed = 1; seed <= 3; ++seed)
            if (check_dense(n_part, seed)) return 1;
    if (chunk_class_cap(256, 1875) != 235 || chunk_class_cap(1, 432) != 2 || chunk_class_cap(9, 100) != 1)
        return fail("chunk_class_cap", 0, 0, 0, 0);
    if (check_rule()) return 1;
    std::printf("ok\n");
    return 0;
}
