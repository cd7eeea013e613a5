// tests/cpp/slot_map_kat.cpp — checks the slot -> pixel map (xraytracer_amd/csrc/slot_map.h,
// host/slot_map.cpp) on its own: tests/test_slot_map.py compiles the two files together, plainly
// and with -fsanitize=address,undefined, and runs the program.
//   * multiplier: for n in {1, 2, 63, 64, 65, 1073 (29 * 37), 1201 (prime), 4096, 60000, 480000,
//     921600} slot_multiplier(n) is coprime to n and smaller than n, and for n >= 2 it is the
//     smallest such A >= round(0.3819660113 * n), found here by a search of its own; n = 1: 0
//   * bijection: for the same n, slot_perm(., A, n) reaches every pixel of [0, n) exactly once, and
//     slot_perm(., 0, n) is the identity
//   * pixel: slot_pixel_at is column q % width of row shard_index + shard_count * (q / width) of the
//     permuted index q, for a whole image and for row shard 3 of 8
//   * spread: for 800 x 600, 800 x 75 (one of 8 row shards), 640 x 480 and 1280 x 720 every aligned
//     run of 64 consecutive slots — a wave of the whole-wave layout; the shard's last, shorter run is
//     left out — touches all 32 of 32 equal bands of the shard's rows
// With the argument "dump W H" it prints the pixel index of every slot of a W x H image under the
// multiplier's map, one per line (tests/test_gpu_interleave.py compares the device's with it).
// Prints "ok" and returns 0, or the first failure and 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "slot_map.h"

using namespace xrt;

static int fail(const char* what, uint32_t n, uint64_t a, uint64_t b) {
    std::printf("FAIL %s (n %u: %llu, %llu)\n", what, n, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

static uint64_t gcd(uint64_t a, uint64_t b) { return b ? gcd(b, a % b) : a; }

static int check_n(uint32_t n) {
    const uint32_t A = slot_multiplier(n);
    if (gcd(A, n) != 1) return fail("coprime", n, A, gcd(A, n));
    if (A >= n) return fail("below n", n, A, 0);
    if (n == 1 && A != 0) return fail("n = 1 is the identity", n, A, 0);
    if (n >= 2) {
        uint64_t want = (uint64_t)(0.3819660113 * (double)n + 0.5);
        if (want < 1) want = 1;
        while (gcd(want, n) != 1) ++want;
        if (A != want) return fail("smallest coprime at or above the golden section", n, A, want);
    }
    std::vector<unsigned char> seen(n, 0);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t q = slot_perm(s, A, n);
        if (q >= n) return fail("pixel out of range", n, s, q);
        if (seen[q]++) return fail("pixel of two slots", n, s, q);
        if (slot_perm(s, 0, n) != s) return fail("multiplier 0 is the identity", n, s, slot_perm(s, 0, n));
    }
    return 0;   // n slots, n distinct pixels below n: every pixel exactly once
}

static int check_pixel(uint32_t width, uint32_t rows, uint32_t shard_index, uint32_t shard_count) {
    const uint32_t n = width * rows, A = slot_multiplier(n);
    for (uint32_t s = 0; s < n; ++s)
        for (uint32_t mul : {0u, A}) {
            const uint32_t q = mul ? (uint32_t)(((uint64_t)s * mul) % n) : s;
            const SlotPixel p = slot_pixel_at(s, mul, n, width, shard_index, shard_count);
            if (p.col != q % width || p.row != shard_index + shard_count * (q / width)) return fail("pixel", n, s, mul);
        }
    return 0;
}

static int check_spread(uint32_t width, uint32_t rows) {
    const uint32_t n = width * rows, A = slot_multiplier(n), kBands = 32;
    for (uint32_t base = 0; base + 64 <= n; base += 64) {
        uint32_t bands = 0;
        for (uint32_t s = base; s < base + 64; ++s) {
            const uint32_t row = slot_perm(s, A, n) / width;
            bands |= 1u << (uint32_t)((uint64_t)row * kBands / rows);
        }
        if (bands != 0xffffffffu) return fail("a wave's 64 slots miss a row band", n, base, bands);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "dump")) {
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]), n = w * h;
        const uint32_t A = slot_multiplier(n);
        for (uint32_t s = 0; s < n; ++s) {
            const SlotPixel p = slot_pixel_at(s, A, n, w, 0, 1);
            std::printf("%u\n", p.col + w * p.row);
        }
        return 0;
    }
    const uint32_t ns[] = {1, 2, 63, 64, 65, 1073, 1201, 4096, 60000, 480000, 921600};
    for (uint32_t n : ns)
        if (check_n(n)) return 1;
    if (check_pixel(37, 29, 0, 1) || check_pixel(64, 12, 3, 8)) return 1;
    const uint32_t shapes[][2] = {{800, 600}, {800, 75}, {640, 480}, {1280, 720}};
    for (const auto& q : shapes)
        if (check_spread(q[0], q[1])) return 1;
    std::printf("ok\n");
    return 0;
}
