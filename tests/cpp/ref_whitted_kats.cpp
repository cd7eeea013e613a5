// ref_whitted_kats.cpp — known answers for the Whitted integrator's geometry from the
// REFERENCE's own geometry.cpp, compiled in place.  TEST INFRASTRUCTURE ONLY.
//
// Build and run by hand (never by a test, never on the GPU machine), with REFFLAGS of
// oracle/Makefile and REF = the reference's Src directory:
//
//   mkdir -p oracle/_ref
//   g++ -std=c++17 -O2 -ffp-contract=off -w -include cfloat -DkEpsilon=FLT_EPSILON -DkInfinity=FLT_MAX \
//       -I$REF -o oracle/_ref/ref_whitted_kats tests/cpp/ref_whitted_kats.cpp $REF/geometry.cpp
//   oracle/_ref/ref_whitted_kats > tests/golden/ref_whitted_kats.json
//
// It includes the reference header geometry.h unmodified; no reference source is copied.  It
// runs reflect, refract, fresnel (ior 1.3, the literal of Src/integrator.h:359,365), normalize,
// Matrix44::multVecMatrix and multDirMatrix on the inputs below and prints every float as its
// uint32 bit pattern:
//   math.in[i]  = I.xyz, N.xyz
//   math.out[i] = reflect.xyz, refract.xyz, kr, normalize(reflect).xyz, normalize(refract).xyz
//   lights[i]   = l2w (16), pos = multVecMatrix(Vec3f(0)) (PointLight's constructor,
//                 Src/light.cpp:115-118), dir = normalize(multDirMatrix((0,0,-1)))
//                 (DistantLight's, :130-134)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "geometry.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct Gen {   // xorshift32
    uint32_t s;
    uint32_t next() {
        s ^= s << 13;
        s ^= s >> 17;
        s ^= s << 5;
        return s;
    }
    float uni(float a, float b) { return a + (b - a) * (float)(next() >> 8) * (1.0f / 16777216.0f); }
    Vec3f unit() {
        for (;;) {
            const Vec3f v(uni(-1, 1), uni(-1, 1), uni(-1, 1));
            const float l = length(v);
            if (l > 0.1f && l <= 1.0f) return v / l;
        }
    }
};

// a unit vector at angle acos(c) from n, in the plane of n and t (t orthogonal to n)
static Vec3f at_cos(const Vec3f& n, const Vec3f& t, float c) {
    const float s = std::sqrt(std::fmax(0.0f, 1.0f - c * c));
    return c * n + s * t;
}

int main() {
    std::vector<std::pair<Vec3f, Vec3f>> in;
    Gen g{0x9e3779b9u};
    for (int i = 0; i < 96; ++i) in.push_back({g.unit(), g.unit()});                       // any angle, either side
    for (int i = 0; i < 24; ++i) in.push_back({g.unit() * g.uni(0.2f, 3.0f), g.unit()});  // non-unit I (metal chains)
    const Vec3f ns[3] = {Vec3f(0, 1, 0), normalize(Vec3f(1, 2, 3)), normalize(Vec3f(-0.3f, 0.1f, -0.9f))};
    for (const Vec3f& n : ns) {
        Vec3f t = cross(n, Vec3f(0.3f, -0.7f, 0.2f));
        t = normalize(t);
        // dot(I, N) = -1, +1 and 0 (as nearly as floats allow), and exactly for the axis normal
        in.push_back({-n, n});
        in.push_back({n, n});
        in.push_back({t, n});
        // grazing, from outside and from inside
        const float graze[] = {1e-7f, 1e-5f, 1e-3f, 1e-2f, 5e-2f};
        for (float c : graze) in.push_back({at_cos(n, t, -c), n}), in.push_back({at_cos(n, t, c), n});
        // the total-internal-reflection boundary from inside: sin(theta) * 1.3 = 1, i.e.
        // cos(theta) = sqrt(1 - 1 / 1.69), stepped through it in ulps and in small offsets
        const float cc = std::sqrt(1.0f - 1.0f / (1.3f * 1.3f));
        float c = cc;
        for (int k = 0; k < 6; ++k) c = std::nextafter(c, 0.0f);
        for (int k = 0; k < 13; ++k, c = std::nextafter(c, 1.0f)) in.push_back({at_cos(n, t, c), n});
        const float off[] = {-1e-2f, -1e-3f, -1e-4f, -1e-5f, 1e-5f, 1e-4f, 1e-3f, 1e-2f};
        for (float d : off) in.push_back({at_cos(n, t, cc + d), n});
        // rays from inside at steeper angles
        const float inside[] = {0.7f, 0.8f, 0.9f, 0.99f, 0.999999f};
        for (float ci : inside) in.push_back({at_cos(n, t, ci), n});
    }
    in.push_back({Vec3f(0, 0, -1), Vec3f(0, 0, 1)});
    in.push_back({Vec3f(0, 0, 1), Vec3f(0, 0, 1)});
    in.push_back({Vec3f(1, 0, 0), Vec3f(0, 0, 1)});

    std::printf("{\"_provenance\": \"tests/cpp/ref_whitted_kats.cpp compiled against the reference's Src/geometry.cpp "
                "and geometry.h in place (g++ -O2 -ffp-contract=off, REFFLAGS of oracle/Makefile); floats as uint32 bit "
                "patterns; ior 1.3f\",\n\"math\": {\"in\": [");
    for (size_t i = 0; i < in.size(); ++i) {
        const Vec3f &I = in[i].first, &N = in[i].second;
        std::printf("%s[%u,%u,%u,%u,%u,%u]", i ? "," : "", bits(I[0]), bits(I[1]), bits(I[2]), bits(N[0]), bits(N[1]),
                    bits(N[2]));
    }
    std::printf("],\n\"out\": [");
    for (size_t i = 0; i < in.size(); ++i) {
        const Vec3f &I = in[i].first, &N = in[i].second;
        const Vec3f rl = reflect(I, N), rr = refract(I, N, 1.3);
        float kr;
        fresnel(I, N, 1.3, kr);
        const Vec3f nl = normalize(rl), nr = normalize(rr);
        std::printf("%s[%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u]", i ? "," : "", bits(rl[0]), bits(rl[1]), bits(rl[2]),
                    bits(rr[0]), bits(rr[1]), bits(rr[2]), bits(kr), bits(nl[0]), bits(nl[1]), bits(nl[2]), bits(nr[0]),
                    bits(nr[1]), bits(nr[2]));
    }
    std::printf("]},\n\"lights\": [");
    std::vector<Matrix44f> ms;
    ms.push_back(Matrix44f(0.95292, 0.289503, 0.0901785, 0, -0.0960954, 0.5704, -0.815727, 0, -0.287593, 0.768656, 0.571365,
                           0, 0, 0, 0, 1));                                                  // example.cpp:59-62
    ms.push_back(Matrix44f(1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 5.0, 5.0, -1.0, 1.0));   // :65-69
    for (int i = 0; i < 6; ++i) {   // rotations with scale and translation; two with w != 1
        const Vec3f a = g.unit(), b = normalize(cross(a, g.unit())), c = cross(a, b);
        const float s = g.uni(0.5f, 3.0f), w = i < 4 ? 1.0f : g.uni(0.5f, 2.0f);
        ms.push_back(Matrix44f(a[0] * s, a[1] * s, a[2] * s, 0, b[0] * s, b[1] * s, b[2] * s, 0, c[0] * s, c[1] * s, c[2] * s,
                               0, g.uni(-9, 9), g.uni(-9, 9), g.uni(-9, 9), w));
    }
    for (size_t i = 0; i < ms.size(); ++i) {
        Vec3f pos, dir;
        ms[i].multVecMatrix(Vec3f(0), pos);
        ms[i].multDirMatrix(Vec3f(0, 0, -1), dir);
        dir = normalize(dir);
        std::printf("%s{\"l2w\": [", i ? ",\n" : "");
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) std::printf("%s%u", r + c ? "," : "", bits(ms[i][r][c]));
        std::printf("], \"pos\": [%u,%u,%u], \"dir\": [%u,%u,%u]}", bits(pos[0]), bits(pos[1]), bits(pos[2]), bits(dir[0]),
                    bits(dir[1]), bits(dir[2]));
    }
    std::printf("]}\n");
    return 0;
}
