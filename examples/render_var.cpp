// examples/render_var.cpp — render with the per-pixel sample variance, guide buffers,
// variance-guided denoise: examples/denoise_var.cpp with the variance the filter reads taken from
// the pixels' own samples (HipRenderer::renderVariance) instead of estimated from the frame.  The
// scene of examples/denoise.cpp (the 30 x 30 plane of cube.obj at y = -2.2, the unit sphere, camera
// at (0, 0, 8), FOV 60, a 2 x 2 QuadLight at y = 4 facing down) under GIIntegrator(3) at a low
// sample count (at least 2).  Both frames go through gammaCorrection(1.2) and writePPM.
//
//   render_var [width height spp out_prefix]     -> out_prefix.noisy.ppm, out_prefix.denoised.ppm
//   render_var width height spp out_prefix fused -> the same two files through the fused schedule
//       (renderVariance's last argument, XRT_FLAG_VAR_FUSED: same frame and plane), and the frame and the
//       plane as they were rendered, raw float32: out_prefix.frame.raw, out_prefix.variance.raw
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
    const uint32_t n_samples = argc > 3 ? (uint32_t)atoi(argv[3]) : 4;
    const std::string out = argc > 4 ? argv[4] : "render_var";
    const bool fused = argc > 5 && std::string(argv[5]) == "fused";
    const uint32_t max_depth = 3;

    const float aspect_ratio = static_cast<float>(width) / height;
    const Matrix44f c2w(1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 8.0, 1);
    const auto camera = std::make_unique<PinholeCamera>(aspect_ratio, c2w, 60.0f);

    const auto material = std::make_unique<Lambert>(Vec3f(0.58));
    const auto plane_material = std::make_unique<Lambert>(Vec3f(1.0));
    Scene scene;
    scene.addObj("plane", std::make_unique<Mesh>(plane(), plane_material.get(), nullptr));
    scene.addObj("sphere_diffuse", std::make_unique<Sphere>(Vec3f(0.0), 1.0f, material.get(), nullptr));
    scene.addAreaLight("QuadLight", std::make_unique<QuadLight>(Vec3f(1.0, 4.0, -1.0), Vec3f(1.0, 4.0, 1.0), Vec3f(-1.0, 4.0, -1.0),
                                                                Matrix44f(), 25.0f * Vec3f(1.0, 1.0, 1.0)));
    scene.build();

    const auto integrator = std::make_unique<GIIntegrator>(max_depth);
    auto renderer = std::make_unique<HipRenderer>(n_samples, camera.get(), integrator.get());
    Image image(width, height);
    std::vector<float> variance;
    renderer->renderVariance(scene, Sampler::SamplerType::Uniform, image, variance, fused);
    if (renderer->lastStatus() != 0) {
        std::fprintf(stderr, "renderVariance failed: %s\n", renderer->lastError().c_str());
        return 2;
    }
    if (fused) {
        std::printf("schedule %llu\n", (unsigned long long)renderer->lastStats().schedule);
        FILE* ff = std::fopen((out + ".frame.raw").c_str(), "wb");
        FILE* fv = std::fopen((out + ".variance.raw").c_str(), "wb");
        const bool ok = ff && fv && std::fwrite(image.data(), sizeof(float), 3 * variance.size(), ff) == 3 * variance.size() &&
                        std::fwrite(variance.data(), sizeof(float), variance.size(), fv) == variance.size();
        if (ff) std::fclose(ff);
        if (fv) std::fclose(fv);
        if (!ok) return 3;
    }
    double mean_sample_variance = 0.0;
    for (float v : variance) mean_sample_variance += v;
    const double render_ms = renderer->lastStats().wall_ms;
    GuideImages g(width, height);
    renderer->renderGuides(scene, g);
    if (renderer->lastStatus() != 0) {
        std::fprintf(stderr, "renderGuides failed: %s\n", renderer->lastError().c_str());
        return 2;
    }
    const double guides_ms = renderer->lastStats().wall_ms;

    Image noisy = image;
    DenoiseVarSettings settings;   // 4 iterations, 4 standard deviations; sigma_depth stays off: it is in world units
    renderer->denoiseVar(image, g, variance, settings, &variance);
    if (renderer->lastStatus() != 0) {
        std::fprintf(stderr, "denoiseVar failed: %s\n", renderer->lastError().c_str());
        return 2;
    }
    const xrt_denoise_stats& ds = renderer->lastDenoiseStats();
    double mean_variance = 0.0;
    for (float v : variance) mean_variance += v;
    std::printf("%ux%u x %u spp: render %.2f ms, guides %.2f ms, denoise %.2f ms (%u launches, %u tiled + %u direct iterations), "
                "mean sample variance %.3g, left %.3g\n",
                width, height, n_samples, render_ms, guides_ms, ds.wall_ms, ds.launches, ds.tiled_iterations,
                ds.direct_iterations, mean_sample_variance / (double)variance.size(), mean_variance / (double)variance.size());

    noisy.gammaCorrection(1.2f);
    image.gammaCorrection(1.2f);
    return noisy.writePPM(out + ".noisy.ppm") && image.writePPM(out + ".denoised.ppm") ? 0 : 3;
}
