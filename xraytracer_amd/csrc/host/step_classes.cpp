// host/step_classes.cpp — the merged trace's per-object kernel-argument records, grouped into
// classes of equal triangle count (wavefront.h StepObjs).  Plain host code: tests/cpp/
// step_classes_kat.cpp compiles it on its own.
//
// The order of the records changes no result: a record's `first` still indexes the scene's
// triangle array, closest hits merge by the minimum of (t bits, triangle index) and occlusion
// by an or, both order-independent.
#include <cstring>

#include "../wavefront.h"

namespace xrt {

void build_step_objs(const DObjBox* boxes, const DObjPlane* planes, int n, StepObjs& SO) {
    std::memset(&SO, 0, sizeof(SO));
    SO.n = n;
    auto count_of = [&](int i) { return (uint32_t)(boxes[i].count_occ & 0x7fffffff); };
    int at = 0;
    for (int lead = 0; lead < n; ++lead) {
        const uint32_t c = count_of(lead);
        bool seen = false;   // an earlier object opened this count's class
        for (int i = 0; i < lead && !seen; ++i) seen = XRT_TRACE_CLASSES && count_of(i) == c;
        if (seen) continue;
        StepClass& K = SO.cls[SO.n_cls++];
        K.c = c;
        // ceil(2^32 / c): floor(j * magic / 2^32) = j / c for j * c < 2^32
        K.magic = c > 1 ? (uint32_t)(((1ull << 32) + c - 1) / c) : 0u;
        K.begin = (uint32_t)at;
        for (int i = lead; i < n; ++i) {
            if (count_of(i) != c || (!XRT_TRACE_CLASSES && i != lead)) continue;
            StepObj& o = SO.o[at++];
            o.axis = planes[i].axis;
            o.plane = planes[i].c;
            for (int q = 0; q < 3; ++q) o.bmin[q] = boxes[i].bmin[q], o.bmax[q] = boxes[i].bmax[q];
            o.first = boxes[i].first;
            o.occluder = boxes[i].count_occ < 0 ? 1u : 0u;
        }
        K.end = (uint32_t)at;
    }
}

}  // namespace xrt
