// tests/cpp/step_groups_kat.cpp — checks the partition groups of the merged schedule's step
// launches (xraytracer_amd/csrc/step_groups.h, host/step_groups.cpp) on their own:
// tests/test_step_groups.py compiles the two files together, plainly and with
// -fsanitize=address,undefined, and runs the program.  For n_part in {8, 16, 24, 232, 256} and
// G in {1, 2, 3}:
//   * eligibility is n_part >= 8 * G (all these n_part are multiples of 8), and false for a count
//     that is no multiple of 8 when G > 1; step_groups_for gives the most eligible groups up to `want`
//   * where eligible, the groups' partitions (step_group_part over step_group_parts) are disjoint
//     and cover every partition, each exactly once
//   * each group is whole octets: a multiple of 8 partitions, local octet o the partitions
//     8 * q .. 8 * q + 7 of one global octet q, in order
//   * the XCD residue is preserved: p % 8 == lp % 8, so a block b with lp = b % parts has
//     p % 8 == b % 8
//   * step_group_of names the group that holds the partition; step_group_arg packs g, G and the
//     group's partition count as the kernel unpacks them
//   * G = 1 is the identity over any n_part (also those below 8)
// Prints "ok" and returns 0, or the first failure and 1.
#include <cstdio>
#include <vector>

#include "step_groups.h"

using namespace xrt;

static int fail(const char* what, uint32_t n_part, uint32_t G, uint32_t a, uint32_t b) {
    std::printf("FAIL %s (n_part %u, G %u: %u, %u)\n", what, n_part, G, a, b);
    return 1;
}

static int check(uint32_t n_part, uint32_t G) {
    const bool want = G == 1 || (n_part % 8 == 0 && n_part >= 8 * G);
    if (step_groups_eligible(n_part, G) != want) return fail("eligibility", n_part, G, want, 0);
    if (!want) return 0;
    std::vector<int> seen(n_part, 0);
    uint32_t total = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t np = G == 1 ? n_part : step_group_parts(n_part, G, g);
        if (G > 1 && (np % 8 != 0 || np == 0)) return fail("whole octets", n_part, G, g, np);
        const uint32_t arg = step_group_arg(n_part, G, g);
        if ((arg & 15u) != g || ((arg >> 4) & 15u) != G || (arg >> 8) != np) return fail("packed argument", n_part, G, g, arg);
        for (uint32_t lp = 0; lp < np; ++lp) {
            const uint32_t p = step_group_part(G, g, lp);
            if (p >= n_part) return fail("partition out of range", n_part, G, lp, p);
            if (seen[p]++) return fail("partition in two groups", n_part, G, lp, p);
            if (p % 8 != lp % 8) return fail("XCD residue", n_part, G, lp, p);
            if (step_group_of(G, p) != g) return fail("group of partition", n_part, G, p, g);
            if (p / 8 != step_group_part(G, g, lp & ~7u) / 8) return fail("octet split", n_part, G, lp, p);
            if (lp >= 8 && p <= step_group_part(G, g, lp - 8)) return fail("octet order", n_part, G, lp, p);
            if (G == 1 && p != lp) return fail("one group is the identity", n_part, G, lp, p);
        }
        total += np;
    }
    if (total != n_part) return fail("cover", n_part, G, total, 0);
    for (uint32_t p = 0; p < n_part; ++p)
        if (seen[p] != 1) return fail("partition missing", n_part, G, p, (uint32_t)seen[p]);
    return 0;
}

int main() {
    const uint32_t parts[] = {8, 16, 24, 232, 256};
    for (uint32_t n_part : parts)
        for (uint32_t G = 1; G <= 3; ++G)
            if (check(n_part, G)) return 1;
    // below 8 * G, and counts that are no multiple of 8 (plan_render gives those only below 8)
    for (uint32_t n_part = 1; n_part < 8; ++n_part)
        for (uint32_t G = 1; G <= 3; ++G)
            if (check(n_part, G)) return 1;
    if (step_groups_eligible(8, 2) || step_groups_eligible(16, 3) || step_groups_eligible(20, 2) ||
        step_groups_eligible(256, 4) || step_groups_eligible(256, 0))
        return fail("eligible", 0, 0, 0, 0);
    if (!step_groups_eligible(16, 2) || !step_groups_eligible(24, 3) || !step_groups_eligible(5, 1))
        return fail("not eligible", 0, 0, 0, 0);
    // the most eligible groups up to `want`
    const uint32_t cases[][3] = {{8, 3, 1},  {8, 2, 1},   {16, 3, 2}, {16, 2, 2}, {24, 3, 3}, {24, 2, 2}, {232, 3, 3},
                                 {256, 1, 1}, {256, 7, 3}, {5, 3, 1},  {1, 2, 1},  {16, 0, 1}};
    for (const auto& q : cases)
        if (step_groups_for(q[0], q[1]) != q[2]) return fail("step_groups_for", q[0], q[1], step_groups_for(q[0], q[1]), q[2]);
    std::printf("ok\n");
    return 0;
}
