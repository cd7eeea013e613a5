// slot_map.h — which pixel a path slot renders: the one definition every kernel,
// the host and the tests share.
//
// A shard of n slots owns the pixels of its rows in row-major order, pixel q at column q % width
// of row shard_index + shard_count * (q / width).  Slot s renders pixel q = slot_perm(s, mul, n):
//   mul == 0  q = s, the row-major map (every schedule but the interleaved merged one);
//   mul != 0  q = s * mul mod n with gcd(mul, n) = 1, a bijection of [0, n) that sends 64
//             consecutive slots — one wave of the merged schedule's whole-wave layout — to pixels
//             spread over the whole shard, so every wave's work is a sample of the image's and the
//             waves of a launch cost about alike.
// A slot's path depends on its pixel and its own RNG stream only (seed col + width * row), so the
// map changes no pixel and no per-pixel counter; all per-slot state stays indexed by slot (coalesced),
// only the framebuffer pixel is scattered.  The multiplier is the host's choice (host/slot_map.cpp,
// plain host code, tests/cpp/slot_map_kat.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define XRT_SLOT_FN __host__ __device__ inline
#else
#define XRT_SLOT_FN inline
#endif

namespace xrt {

struct SlotPixel {
    uint32_t col, row;
};

// the shard-local pixel index of slot s
XRT_SLOT_FN uint32_t slot_perm(uint32_t s, uint32_t mul, uint32_t n) {
    return mul ? (uint32_t)(((uint64_t)s * mul) % n) : s;
}
// ... and its column and image row
XRT_SLOT_FN SlotPixel slot_pixel_at(uint32_t s, uint32_t mul, uint32_t n, uint32_t width, uint32_t shard_index,
                                    uint32_t shard_count) {
    const uint32_t q = slot_perm(s, mul, n);
    return {q % width, shard_index + shard_count * (q / width)};
}

// host/slot_map.cpp.  The interleaving multiplier of a shard of n slots: the smallest
// A >= round(0.3819660113 * n) (the golden section: consecutive slots land far apart, and so do
// slots 2, 3, 5, 8, ... apart) with gcd(A, n) == 1; 0 (the row-major map) for n <= 1.  A < n for n >= 2.
uint32_t slot_multiplier(uint32_t n);

}  // namespace xrt
