// examples/progressive.cpp — a frame that converges on screen: the Cornell box of
// examples/cornellbox.cpp under GIIntegrator(3), rendered in passes through HipRenderer's progressive
// session (beginProgressive / addSamples / progressiveFrame).  Every pass continues the pixels' sample
// streams, so the frame after the last pass is, bit for bit, one render at the passes' total sample
// count — and the passes together cost that many samples, not the sum of their running totals.
// After each pass the frame so far and its variance-guided denoise (HipRenderer::denoiseVar over the
// session's own variance plane, from 2 samples on; estimated from the frame before that) go through
// gammaCorrection(1.2) and writePPM.
//
//   progressive [width height out_prefix pass ...]     passes default to 1 3 12 48
//     -> out_prefix.<spp>.ppm, out_prefix.<spp>.denoised.ppm for every running total <spp>
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

#ifndef DATA_DIR
#define DATA_DIR "xraytracer_amd/data/"
#endif

int main(int argc, char** argv) {
    const uint32_t width = argc > 1 ? (uint32_t)atoi(argv[1]) : 780;
    const uint32_t height = argc > 2 ? (uint32_t)atoi(argv[2]) : 585;
    const std::string out = argc > 3 ? argv[3] : "progressive";
    std::vector<uint32_t> passes;
    for (int a = 4; a < argc; ++a) passes.push_back((uint32_t)atoi(argv[a]));
    if (passes.empty()) passes = {1, 3, 12, 48};
    const uint32_t max_depth = 3;

    const float aspect_ratio = static_cast<float>(width) / height;
    const Matrix44f c2w(-1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, -1.0, 0, 278, 274.4, -750.0, 1);
    const auto camera = std::make_unique<PinholeCamera>(aspect_ratio, c2w, 60.0f);

    Scene scene;
    const char* env = std::getenv("XRT_DATA_DIR");
    const std::string dataDir = env ? env : DATA_DIR;
    if (!scene.loadObj(dataDir + "cornell_box.obj")) {
        std::fprintf(stderr, "%s\n", scene.lastError().c_str());
        return 1;
    }
    scene.addAreaLight("QuadLight", std::make_unique<QuadLight>(Vec3f(343.0, 548.0, 227.0), Vec3f(343.0, 548.0, 332.0),
                                                                Vec3f(213.0, 548.0, 227.0), Matrix44f(),
                                                                25.0f * Vec3f(1.0, 1.0, 1.0)));
    scene.build();

    const auto integrator = std::make_unique<GIIntegrator>(max_depth);
    // n_samples serves the guide buffers only: a session takes its sample counts pass by pass
    auto renderer = std::make_unique<HipRenderer>(4, camera.get(), integrator.get());
    auto failed = [&](const char* what) {
        if (renderer->lastStatus() == 0) return false;
        std::fprintf(stderr, "%s failed: %s\n", what, renderer->lastError().c_str());
        return true;
    };
    // the guide buffers first: renderGuides is a render, and a render ends a session
    GuideImages g(width, height);
    renderer->renderGuides(scene, g);
    if (failed("renderGuides")) return 2;

    Image image(width, height);
    renderer->beginProgressive(scene, Sampler::SamplerType::Uniform, image, true);
    if (failed("beginProgressive")) return 2;
    for (uint32_t n : passes) {
        renderer->addSamples(n);
        if (failed("addSamples")) return 2;
        const xrt_stats st = renderer->lastStats();
        const uint32_t done = renderer->samplesDone();
        std::vector<float> variance;
        renderer->progressiveFrame(image, done >= 2 ? &variance : nullptr);
        if (failed("progressiveFrame")) return 2;
        Image clean = image;
        if (done >= 2) renderer->denoiseVar(clean, g, variance);
        else renderer->denoiseVar(clean, g);
        if (failed("denoiseVar")) return 2;
        std::printf("pass +%u: spp_done %u, %.2f ms, samples %llu segments %llu shadow_rays %llu draws %llu rejected %llu\n", n,
                    done, st.wall_ms, (unsigned long long)st.samples, (unsigned long long)st.segments,
                    (unsigned long long)st.shadow_rays, (unsigned long long)st.draws, (unsigned long long)st.rejected);
        Image noisy = image;
        noisy.gammaCorrection(1.2f);
        clean.gammaCorrection(1.2f);
        const std::string base = out + "." + std::to_string(done);
        if (!noisy.writePPM(base + ".ppm") || !clean.writePPM(base + ".denoised.ppm")) return 3;
    }
    renderer->endProgressive();
    return 0;
}
