// host/slot_map.cpp — the interleaving multiplier of the slot -> pixel map (slot_map.h has the
// map itself, which the kernels share).  Plain host code: tests/cpp/slot_map_kat.cpp compiles it on
// its own.
//
// The multiplier changes no result: any A coprime to n makes s -> s * A mod n a bijection, and a
// slot's path depends on its own pixel only.  What the choice decides is how evenly 64 consecutive
// slots sample the shard; the golden section spreads every run of consecutive multiples about
// evenly (the three-distance theorem), and tests/cpp/slot_map_kat.cpp checks the spread for the
// image sizes the whole-wave layout runs at.
#include "../slot_map.h"

namespace xrt {

static uint32_t gcd_u32(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t t = a % b;
        a = b, b = t;
    }
    return a;
}

uint32_t slot_multiplier(uint32_t n) {
    if (n <= 1u) return 0u;
    uint64_t a = (uint64_t)(0.3819660113 * (double)n + 0.5);
    if (a < 1u) a = 1u;
    while (a < n && gcd_u32((uint32_t)a, n) != 1u) ++a;
    return a < n ? (uint32_t)a : 1u;   // n - 1 is coprime to n, so the search ends below n
}

}  // namespace xrt
