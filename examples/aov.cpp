// examples/aov.cpp — the guide buffers of examples/whitted.cpp's frame: the example scene (the
// 30 x 30 plane of cube.obj at y = -2.2, the unit sphere, camera at (0, 0, 8), FOV 60) through
// HipRenderer::renderGuides, the planes a denoiser takes beside a low-spp frame.  The shading
// normal is written as the colour 0.5 * (n + 1) and the albedo as it is, both through
// gammaCorrection(1.2) and writePPM; depth and coverage are summarised on stdout.
//
//   aov [width height spp out_prefix]     -> out_prefix.normal.ppm, out_prefix.albedo.ppm
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <xrt/camera.h>
#include <xrt/image.h>
#include <xrt/integrator.h>
#include <xrt/renderer.h>
#include <xrt/scene.h>

// the plane of cube.obj: f v0 v1 v2 v3 -> (v0, v1, v3), (v1, v2, v3) (examples/whitted.cpp)
static std::vector<Primitive> plane() {
    const Vec3f v[4] = {Vec3f(15.0, -2.2, 15.0), Vec3f(15.0, -2.2, -15.0), Vec3f(-15.0, -2.2, -15.0),
                        Vec3f(-15.0, -2.2, 15.0)};
    const std::vector<Vec2f> uv = {Vec2f(0, 0), Vec2f(1, 0), Vec2f(0, 1)};
    const int idx[2][3] = {{0, 1, 3}, {1, 2, 3}};
    std::vector<Primitive> prims;
    for (const auto& t : idx) {
        const std::vector<Vec3f> vs = {v[t[0]], v[t[1]], v[t[2]]};
        const Vec3f n = normalize(cross(vs[1] - vs[0], vs[2] - vs[0]));
        prims.emplace_back(vs, std::vector<Vec3f>{n, n, n}, uv);
    }
    return prims;
}

int main(int argc, char** argv) {
    const uint32_t width = argc > 1 ? (uint32_t)atoi(argv[1]) : 780;
    const uint32_t height = argc > 2 ? (uint32_t)atoi(argv[2]) : 585;
    const uint32_t n_samples = argc > 3 ? (uint32_t)atoi(argv[3]) : 16;
    const std::string out = argc > 4 ? argv[4] : "aov";

    const float aspect_ratio = static_cast<float>(width) / height;
    const Matrix44f c2w(1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 8.0, 1);
    const auto camera = std::make_unique<PinholeCamera>(aspect_ratio, c2w, 60.0f);

    const auto material = std::make_unique<Lambert>(Vec3f(0.58));
    const auto plane_material = std::make_unique<Lambert>(Vec3f(1.0));
    Scene scene;
    scene.addObj("plane", std::make_unique<Mesh>(plane(), plane_material.get(), nullptr));
    scene.addObj("sphere_diffuse", std::make_unique<Sphere>(Vec3f(0.0), 1.0f, material.get(), nullptr));
    scene.build();

    // the guide pass consults no integrator; the Renderer base class still holds one
    const auto integrator = std::make_unique<NormalIntegrator>();
    auto renderer = std::make_unique<HipRenderer>(n_samples, camera.get(), integrator.get());
    GuideImages g(width, height);
    renderer->renderGuides(scene, g);
    if (renderer->lastStatus() != 0) {
        std::fprintf(stderr, "renderGuides failed: %s\n", renderer->lastError().c_str());
        return 2;
    }
    const xrt_stats& st = renderer->lastStats();
    double cover = 0.0, depth = 0.0;
    size_t on_object = 0;
    for (size_t k = 0; k < g.alpha.size(); ++k) cover += g.alpha[k], depth += g.depth[k], on_object += g.object[k] >= 0;
    std::printf("guides %ux%u x %u spp in %.2f ms: %.1f Msamples/s, coverage %.4f, mean hit depth %.4f, %zu pixels on an object\n",
                width, height, n_samples, st.wall_ms, (double)st.samples / st.wall_ms / 1e3, cover / (double)g.alpha.size(),
                cover > 0.0 ? depth / cover : 0.0, on_object);

    // NormalIntegrator's colour for the mean shading normal: 0.5f * (ns + 1.0f)
    for (uint32_t i = 0; i < height; ++i)
        for (uint32_t j = 0; j < width; ++j) g.normal.setPixel(i, j, 0.5f * (g.normal.getPixel(i, j) + 1.0f));
    g.normal.gammaCorrection(1.2f);
    g.albedo.gammaCorrection(1.2f);
    return g.normal.writePPM(out + ".normal.ppm") && g.albedo.writePPM(out + ".albedo.ppm") ? 0 : 3;
}
