// xrt/renderer.h — Renderer (Src/renderer.h:8-20) and HipRenderer, the MI355X backend that
// replaces NormalRenderer / ParallelRenderer (Src/renderer.cpp).  HipRenderer::render has
// the reference's signature and contract: it fills `image` in place with the per-pixel mean
// of n_samples samples (seed j + width*i per pixel, NaN/Inf/negative samples dropped).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "camera.h"
#include "image.h"
#include "integrator.h"
#include "sampler.h"
#include "scene.h"

class Renderer {
public:
    Renderer(Camera* cam, Integrator* inte) : camera(cam), integrator(inte) {}
    virtual ~Renderer() = default;
    virtual void render(const Scene& scene, Sampler::SamplerType st, Image& image) const = 0;

protected:
    const Camera* camera;
    const Integrator* integrator;
};

// First-hit guide buffers of a frame (xrt.h, xrt_render_aov), for a denoiser or compositor:
// sample means of albedo, shading normal, depth (IntersectInfo::t) and coverage over the
// render's own camera rays, and the object index (Scene iteration order, -1 = miss) of sample
// 0.  HipRenderer::renderGuides fills the members that have a size — Images of the frame's
// width x height, vectors of width * height elements in Image::pixels order — and skips empty
// ones; every sized member must have the size `width` x `height` names.
struct GuideImages {
    Image albedo{0, 0}, normal{0, 0};
    std::vector<float> depth, alpha;
    std::vector<int32_t> object;
    uint32_t width = 0, height = 0;   // the frame's size
    GuideImages() = default;
    // every plane, sized
    GuideImages(uint32_t w, uint32_t h)
        : albedo(w, h), normal(w, h), depth((size_t)w * h), alpha((size_t)w * h), object((size_t)w * h), width(w), height(h) {}
};

// The edge-avoiding a-trous filter's settings (xrt.h, xrt_denoise): passes of the 5 x 5 kernel
// with tap spacing 1, 2, 4, ..., and the four edge-stopping widths; a sigma <= 0 turns its term
// off.  sigma_depth is the depth change tolerated per step of tap spacing in the scene's world
// units, so it has no scene-independent default and starts off.  tile = false sends every
// iteration through the direct kernel (same results).
struct DenoiseSettings {
    uint32_t iterations = 3;
    float sigma_color = 2.0f, sigma_normal = 0.5f, sigma_depth = 0.0f, sigma_albedo = 0.2f;
    bool tile = true, timing = false;
};

// The variance-guided filter's settings (xrt.h, xrt_denoise_var): the colour stop is a luminance
// difference in standard deviations of the pixel's own noise, sigma_luminance of them, so it needs
// no tuning to the radiance scale or the iteration count.  The variance is estimated from the frame
// over a window of (2 variance_radius + 1)^2 pixels of the same object (1 .. 3).
struct DenoiseVarSettings {
    uint32_t iterations = 4;
    float sigma_luminance = 4.0f, sigma_normal = 0.5f, sigma_depth = 0.0f, sigma_albedo = 0.2f;
    uint32_t variance_radius = 3;
    bool tile = true, timing = false;
};

struct xrt_ctx;
class HipRenderer : public Renderer {
public:
    HipRenderer(uint32_t spp, Camera* cam, Integrator* inte, int device = 0);
    // ParallelRenderer over several GPUs (Src/renderer.cpp:83-99): the image's rows are
    // interleaved over `devices` and assembled on devices[0] (xrt_create_multi)
    HipRenderer(uint32_t spp, Camera* cam, Integrator* inte, std::vector<int> devices);
    ~HipRenderer() override;
    // Errors are reported like the reference reports them (logged; the image is left as
    // rendered so far); lastStatus()/lastError() expose them to callers that care.
    void render(const Scene& scene, Sampler::SamplerType st, Image& image) const override;
    // render() over a zero Image — `image`'s earlier contents are replaced, not added to — and,
    // beside the frame, the variance of each pixel's mean luminance from the pixel's own samples
    // (xrt.h, xrt_render_var; n_samples must be at least 2): `variance` is resized to width *
    // height in Image::pixels order.  It is what denoiseVar takes as variance_in.  Errors as
    // render() reports them.  fused: the path integrators keep the fused or merged schedule instead
    // of the wavefront (XRT_FLAG_VAR_FUSED); the same frame and plane, sooner.
    void renderVariance(const Scene& scene, Sampler::SamplerType st, Image& image, std::vector<float>& variance,
                        bool fused = false) const;
    // A frame in passes (xrt.h, xrt_progressive_*): beginProgressive seeds a session for `scene` at
    // `image`'s size (the image is not written, n_samples not consulted), every addSamples(n) renders n
    // more samples of each pixel, and progressiveFrame replaces `image` with the mean of the
    // samplesDone() samples so far — bit for bit render() over a zero Image at that many samples.
    // variance = true also sums the luminance moments, so progressiveFrame can fill `variance` as
    // renderVariance does (from 2 samples on).  The session runs the schedule of render() without
    // speculative sample starts and pixel-parallel chains; WhittedIntegrator and a multi-GPU renderer
    // are refused.  Any other render, renderGuides or a new scene ends it; the filters do not.
    // lastStats() after addSamples: path counters of the session so far, timings of that pass.
    // Errors as render() reports them.
    void beginProgressive(const Scene& scene, Sampler::SamplerType st, const Image& image, bool variance = false) const;
    void addSamples(uint32_t n) const;
    void progressiveFrame(Image& image, std::vector<float>* variance = nullptr) const;
    uint32_t samplesDone() const;   // 0 without an open session
    void endProgressive() const;
    // The guide buffers of the frame render() would make of `scene` with this camera and
    // n_samples (the integrator is not consulted); errors as render() reports them.
    void renderGuides(const Scene& scene, GuideImages& guides) const;
    // Filters `image` in place over the planes of `guides` that have a size (the others are
    // passed as NULL: planes of zeros; alpha is not read).  Needs no scene; creates the context
    // if no call has yet.  Errors as render() reports them.
    void denoise(Image& image, const GuideImages& guides, const DenoiseSettings& settings = {}) const;
    // As denoise(), through the variance-guided filter with the variance estimated from `image`;
    // variance_out, when given, is resized to width * height and receives the variance left after
    // the last pass.
    void denoiseVar(Image& image, const GuideImages& guides, const DenoiseVarSettings& settings = {},
                    std::vector<float>* variance_out = nullptr) const;
    // ... with the caller's variance of each pixel's luminance, renderVariance's for instance
    // (width * height elements, finite and >= 0), in place of the estimate; variance_out may be
    // variance_in's vector.
    void denoiseVar(Image& image, const GuideImages& guides, const std::vector<float>& variance_in,
                    const DenoiseVarSettings& settings = {}, std::vector<float>* variance_out = nullptr) const;
    int lastStatus() const { return m_status; }
    const std::string& lastError() const { return m_error; }
    const xrt_stats& lastStats() const { return m_stats; }
    const xrt_denoise_stats& lastDenoiseStats() const { return m_denoise_stats; }

private:
    int context() const;                     // creates the context on first use; XRT_OK or fails with m_error set
    int prepare(const Scene& scene) const;   // context, scene, delta lights, camera; XRT_OK or fails with m_error set
    void fail(int rc, const std::string& msg) const;   // m_status, m_error and a line on stderr
    // the start of denoise() / denoiseVar() (`who`): the guide planes of `guides` that have a size, as
    // the filters read them, and the context; false after fail()
    bool filterInputs(const char* who, const Image& image, const GuideImages& guides, xrt_aov_buffers& in) const;
    // both denoiseVar()s: variance_in null = estimated from the image
    void filterVar(Image& image, const GuideImages& guides, const float* variance_in, const DenoiseVarSettings& settings,
                   std::vector<float>* variance_out) const;
    // the start of render() / renderVariance(): scene, camera and medium uploaded, and p for `image`
    // with this integrator and n_samples; false after a failure (m_status, m_error set)
    bool renderInputs(const Scene& scene, const Image& image, xrt_render_params& p) const;
    const uint32_t n_samples;
    int m_device;
    std::vector<int> m_devices;   // empty: one GPU (m_device)
    mutable xrt_ctx* m_ctx = nullptr;
    mutable int m_status = 0;
    mutable std::string m_error;
    mutable xrt_stats m_stats{};
    mutable xrt_denoise_stats m_denoise_stats{};
};
