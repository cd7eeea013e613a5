// tests/cpp/step_classes_kat.cpp — checks the merged trace's host grouping (xraytracer_amd/csrc/
// host/step_classes.cpp: build_step_objs) on its own: tests/test_step_classes.py compiles the two
// files together, plainly and with -fsanitize=address,undefined, and runs the program.
//   * the classes tile the records: cls[0].begin = 0, cls[k].begin = cls[k - 1].end, the last end = n
//   * every object appears exactly once, with its box, plane, first triangle and occluder flag,
//     in a class of its own triangle count; no two classes share a count
//   * classes in the order in which their counts first appear, objects inside one in scene order
//   * magic: j / c by the multiply the device uses, for every pair index a wave can form
//     (j < 64 lanes * 32 objects * c) and every count an LDS scene can hold
//   * 0, 1 and 32 objects
// Prints "ok" and returns 0, or the first failure and 1.
#include <cstdio>
#include <vector>

#include "wavefront.h"

using namespace xrt;

static int fail(const char* what, int a, int b) {
    std::printf("FAIL %s (%d, %d)\n", what, a, b);
    return 1;
}

static int check(const std::vector<int>& counts) {
    const int n = (int)counts.size();
    std::vector<DObjBox> boxes(n);
    std::vector<DObjPlane> planes(n);
    int first = 0;
    for (int i = 0; i < n; ++i) {
        for (int q = 0; q < 3; ++q) boxes[i].bmin[q] = (float)(10 * i + q), boxes[i].bmax[q] = (float)(10 * i + q + 5);
        boxes[i].first = first;
        boxes[i].count_occ = counts[i] | (i % 3 == 1 ? (int)0x80000000 : 0);
        planes[i].axis = i % 4 - 1, planes[i].c = 0.5f * (float)i;
        first += counts[i];
    }
    StepObjs SO;
    build_step_objs(boxes.data(), planes.data(), n, SO);   // null data() when n = 0: never read
    if (SO.n != n) return fail("n", SO.n, n);
    if (SO.n_cls < 0 || SO.n_cls > kMergedMaxObjs || SO.n_cls > n) return fail("n_cls", SO.n_cls, n);
    std::vector<int> seen(n, 0);
    uint32_t at = 0;
    int order = -1;   // scene index of the previous class's first object
    for (int k = 0; k < SO.n_cls; ++k) {
        const StepClass& K = SO.cls[k];
        if (K.begin != at || K.end <= K.begin || K.end > (uint32_t)n) return fail("class range", k, (int)K.begin);
        at = K.end;
        for (int k2 = 0; k2 < k; ++k2)
            if (XRT_TRACE_CLASSES && SO.cls[k2].c == K.c) return fail("two classes of one count", k2, k);
        if (K.magic != (K.c > 1 ? (uint32_t)(((1ull << 32) + K.c - 1) / K.c) : 0u)) return fail("magic", k, (int)K.magic);
        int prev = -1;
        for (uint32_t r = K.begin; r < K.end; ++r) {
            const StepObj& o = SO.o[r];
            const int i = (int)o.bmin[0] / 10;   // which object the record was made from
            if (i < 0 || i >= n) return fail("record's object", (int)r, i);
            if (seen[i]++) return fail("object twice", (int)r, i);
            if ((uint32_t)counts[i] != K.c) return fail("count in class", i, (int)K.c);
            if (i <= prev) return fail("scene order inside a class", i, prev);
            if (r == K.begin) {
                if (i <= order) return fail("class order", i, order);
                for (int e = 0; e < i; ++e)
                    if (XRT_TRACE_CLASSES && counts[e] == counts[i]) return fail("class opened late", e, i);
                order = i;
            }
            prev = i;
            bool same = o.first == boxes[i].first && o.occluder == (boxes[i].count_occ < 0 ? 1u : 0u) &&
                        o.axis == planes[i].axis && o.plane == planes[i].c;
            for (int q = 0; q < 3; ++q) same = same && o.bmin[q] == boxes[i].bmin[q] && o.bmax[q] == boxes[i].bmax[q];
            if (!same) return fail("record's fields", (int)r, i);
        }
    }
    if (at != (uint32_t)n) return fail("classes end", (int)at, n);
    for (int i = 0; i < n; ++i)
        if (seen[i] != 1) return fail("object missing", i, seen[i]);
    return 0;
}

// the device's split of pair j (merged_trace, merged.h)
static uint32_t ray_of(uint32_t j, uint32_t c, uint32_t magic) {
    return c == 1u ? j : c == 2u ? j >> 1 : (uint32_t)(((uint64_t)j * magic) >> 32);
}

int main() {
    std::vector<std::vector<int>> cases = {
        {},                                   // no object
        {7},                                  // one
        {2, 2, 2, 6, 10, 10, 2, 2, 2},        // the Cornell box's counts: classes of 2, 6 and 10
        {1, 3, 1, 1},                         // single triangles beside a 3-triangle object
        {5, 4, 3, 2, 1},                      // all different
        {12, 1, 12, 256, 1, 12, 256, 3},
        std::vector<int>(32, 2),              // 32 of one count
    };
    std::vector<int> all;                     // 32 different counts
    for (int i = 0; i < kMergedMaxObjs; ++i) all.push_back(kMergedMaxObjs - i);
    cases.push_back(all);
    std::vector<int> mixed;                   // 32 objects of 5 counts, interleaved
    for (int i = 0; i < kMergedMaxObjs; ++i) mixed.push_back(1 + (i * 7) % 5);
    cases.push_back(mixed);
    for (size_t q = 0; q < cases.size(); ++q)
        if (check(cases[q])) return std::printf("in case %zu\n", q), 1;
    // every count a record can carry: the counts of scenes whose triangles fit LDS
    for (int c = 1; c <= kSmallTris; c = c < 260 ? c + 1 : c + 97) {
        const std::vector<int> one = {c};
        std::vector<DObjBox> box(1);
        std::vector<DObjPlane> plane(1);
        box[0] = DObjBox{{0, 0, 0}, 0, {1, 1, 1}, c};
        plane[0] = DObjPlane{-1, 0.0f};
        StepObjs SO;
        build_step_objs(box.data(), plane.data(), 1, SO);
        if (SO.n_cls != 1 || SO.cls[0].c != (uint32_t)c) return fail("single class", c, SO.n_cls);
        const uint32_t pairs = 64u * (uint32_t)kMergedMaxObjs * (uint32_t)c;
        for (uint32_t j = 0; j < pairs; ++j)
            if (ray_of(j, (uint32_t)c, SO.cls[0].magic) != j / (uint32_t)c) return fail("j / c", (int)j, c);
    }
    std::printf("ok\n");
    return 0;
}
