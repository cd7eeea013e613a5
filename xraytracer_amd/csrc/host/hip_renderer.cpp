// hip_renderer.cpp — HipRenderer: the Renderer subclass that drops in where the reference
// uses NormalRenderer / ParallelRenderer (Src/renderer.cpp).  It flattens the Scene,
// uploads it, and runs the MI355X wavefront through the C ABI (include/xrt.h).
#include <cstdio>
#include <cstring>

#include "xrt.h"
#include "xrt/renderer.h"

HipRenderer::HipRenderer(uint32_t spp, Camera* cam, Integrator* inte, int device)
    : Renderer(cam, inte), n_samples(spp), m_device(device) {}

HipRenderer::HipRenderer(uint32_t spp, Camera* cam, Integrator* inte, std::vector<int> devices)
    : Renderer(cam, inte), n_samples(spp), m_device(devices.empty() ? 0 : devices[0]), m_devices(std::move(devices)) {}

HipRenderer::~HipRenderer() {
    if (m_ctx) xrt_destroy(m_ctx);
}

int HipRenderer::context() const {
    m_status = XRT_OK;
    m_error.clear();
    if (m_ctx) return XRT_OK;
    const int rc = m_devices.size() > 1 ? xrt_create_multi(m_devices.data(), (int)m_devices.size(), &m_ctx)
                                        : xrt_create(m_device, &m_ctx);
    if (rc != XRT_OK) {
        m_status = rc;
        m_error = std::string("xrt_create: ") + xrt_last_error(nullptr);
        std::fprintf(stderr, "[HipRenderer] %s\n", m_error.c_str());
    }
    return rc;
}

int HipRenderer::prepare(const Scene& scene) const {
    auto fail = [&](int rc, const char* what) {
        m_status = rc;
        m_error = std::string(what) + ": " + (m_ctx ? xrt_last_error(m_ctx) : xrt_last_error(nullptr));
        std::fprintf(stderr, "[HipRenderer] %s\n", m_error.c_str());
        return rc;
    };
    int rc = context();
    if (rc != XRT_OK) return rc;
    xrt_scene_desc desc;
    rc = scene.flatten(&desc);
    if (rc != XRT_OK) return fail(rc, "Scene::flatten");
    if ((rc = xrt_upload_scene(m_ctx, &desc)) != XRT_OK) return fail(rc, "xrt_upload_scene");

    const std::vector<xrt_delta_light>& dl = scene.flattenDeltaLights();
    if ((rc = xrt_set_delta_lights(m_ctx, dl.data(), (uint32_t)dl.size())) != XRT_OK)
        return fail(rc, "xrt_set_delta_lights");

    const Matrix44f& m = camera->cameraToWorld();
    float c2w[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) c2w[4 * r + c] = m[r][c];
    if ((rc = xrt_set_camera(m_ctx, c2w, camera->scale(), camera->aspectRatio())) != XRT_OK)
        return fail(rc, "xrt_set_camera");
    return XRT_OK;
}

void HipRenderer::fail(int rc, const std::string& msg) const {
    m_status = rc;
    m_error = msg;
    std::fprintf(stderr, "[HipRenderer] %s\n", m_error.c_str());
}

void HipRenderer::renderGuides(const Scene& scene, GuideImages& g) const {
    // a member takes part when it has a size, and then it has the frame's
    const size_t npix = (size_t)g.width * g.height;
    const size_t na = (size_t)g.albedo.getWidth() * g.albedo.getHeight(), nn = (size_t)g.normal.getWidth() * g.normal.getHeight();
    const bool image_ok = (!na || (g.albedo.getWidth() == g.width && g.albedo.getHeight() == g.height)) &&
                          (!nn || (g.normal.getWidth() == g.width && g.normal.getHeight() == g.height));
    for (size_t n : {g.depth.size(), g.alpha.size(), g.object.size()})
        if (npix == 0 || !image_ok || (n && n != npix))
            return fail(XRT_ERR_INVALID, "renderGuides: every sized member of GuideImages must be width x height");
    if (prepare(scene) != XRT_OK) return;
    xrt_render_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = g.width, p.height = g.height, p.spp = n_samples;
    p.shard_index = 0, p.shard_count = 1;
    const xrt_aov_buffers out{na ? g.albedo.data() : nullptr, nn ? g.normal.data() : nullptr,
                              g.depth.empty() ? nullptr : g.depth.data(), g.alpha.empty() ? nullptr : g.alpha.data(),
                              g.object.empty() ? nullptr : g.object.data()};
    const int rc = xrt_render_aov(m_ctx, &p, &out, &m_stats);
    if (rc != XRT_OK) fail(rc, std::string("xrt_render_aov: ") + xrt_last_error(m_ctx));
}

// A guide plane takes part when it has a size, and then it has the image's.  xrt_aov_buffers serves
// outputs elsewhere; the filters only read through it.
bool HipRenderer::filterInputs(const char* who, const Image& image, const GuideImages& g, xrt_aov_buffers& in) const {
    const uint32_t w = image.getWidth(), h = image.getHeight();
    const size_t npix = (size_t)w * h;
    const size_t na = (size_t)g.albedo.getWidth() * g.albedo.getHeight(), nn = (size_t)g.normal.getWidth() * g.normal.getHeight();
    if ((na && (g.albedo.getWidth() != w || g.albedo.getHeight() != h)) ||
        (nn && (g.normal.getWidth() != w || g.normal.getHeight() != h)) || (!g.depth.empty() && g.depth.size() != npix) ||
        (!g.object.empty() && g.object.size() != npix)) {
        fail(XRT_ERR_INVALID, std::string(who) + ": every sized member of GuideImages must have the image's size");
        return false;
    }
    in = xrt_aov_buffers{na ? const_cast<float*>(g.albedo.data()) : nullptr, nn ? const_cast<float*>(g.normal.data()) : nullptr,
                         g.depth.empty() ? nullptr : const_cast<float*>(g.depth.data()), nullptr,
                         g.object.empty() ? nullptr : const_cast<int32_t*>(g.object.data())};
    return context() == XRT_OK;
}

void HipRenderer::denoise(Image& image, const GuideImages& g, const DenoiseSettings& s) const {
    xrt_aov_buffers in;
    if (!filterInputs("denoise", image, g, in)) return;
    xrt_denoise_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = image.getWidth(), p.height = image.getHeight(), p.iterations = s.iterations;
    p.sigma_color = s.sigma_color, p.sigma_normal = s.sigma_normal, p.sigma_depth = s.sigma_depth, p.sigma_albedo = s.sigma_albedo;
    p.flags = (s.timing ? XRT_DENOISE_TIMING : 0u) | (s.tile ? 0u : XRT_DENOISE_NO_TILE);
    const int rc = xrt_denoise(m_ctx, &p, image.data(), &in, image.data(), &m_denoise_stats);
    if (rc != XRT_OK) fail(rc, std::string("xrt_denoise: ") + xrt_last_error(m_ctx));
}

void HipRenderer::denoiseVar(Image& image, const GuideImages& g, const DenoiseVarSettings& s, std::vector<float>* variance_out) const {
    filterVar(image, g, nullptr, s, variance_out);
}

void HipRenderer::denoiseVar(Image& image, const GuideImages& g, const std::vector<float>& variance_in, const DenoiseVarSettings& s,
                             std::vector<float>* variance_out) const {
    if (variance_in.size() != (size_t)image.getWidth() * image.getHeight())
        return fail(XRT_ERR_INVALID, "denoiseVar: variance_in must have width * height elements");
    filterVar(image, g, variance_in.data(), s, variance_out);
}

void HipRenderer::filterVar(Image& image, const GuideImages& g, const float* variance_in, const DenoiseVarSettings& s,
                            std::vector<float>* variance_out) const {
    xrt_aov_buffers in;
    if (!filterInputs("denoiseVar", image, g, in)) return;
    xrt_denoise_var_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = image.getWidth(), p.height = image.getHeight(), p.iterations = s.iterations;
    p.sigma_luminance = s.sigma_luminance, p.sigma_normal = s.sigma_normal, p.sigma_depth = s.sigma_depth;
    p.sigma_albedo = s.sigma_albedo, p.variance_radius = s.variance_radius;
    p.flags = (s.timing ? XRT_DENOISE_TIMING : 0u) | (s.tile ? 0u : XRT_DENOISE_NO_TILE);
    // variance_out may be variance_in's vector: the filter works in place
    if (variance_out && variance_out->data() != variance_in) variance_out->assign((size_t)p.width * p.height, 0.0f);
    const int rc = xrt_denoise_var(m_ctx, &p, image.data(), variance_in, &in, image.data(),
                                   variance_out ? variance_out->data() : nullptr, &m_denoise_stats);
    if (rc != XRT_OK) fail(rc, std::string("xrt_denoise_var: ") + xrt_last_error(m_ctx));
}

void HipRenderer::render(const Scene& scene, Sampler::SamplerType, Image& image) const {
    xrt_render_params p;
    if (!renderInputs(scene, image, p)) return;
    p.flags |= XRT_FLAG_ACCUMULATE;   // samples are added to the Image in place (Src/renderer.cpp:75, 98)
    const int rc = xrt_render(m_ctx, &p, image.data(), &m_stats);
    if (rc != XRT_OK) fail(rc, std::string("xrt_render: ") + xrt_last_error(m_ctx));
}

void HipRenderer::renderVariance(const Scene& scene, Sampler::SamplerType, Image& image, std::vector<float>& variance,
                                 bool fused) const {
    xrt_render_params p;
    variance.assign((size_t)image.getWidth() * image.getHeight(), 0.0f);
    if (!renderInputs(scene, image, p)) return;
    if (fused) p.flags |= XRT_FLAG_VAR_FUSED;
    const int rc = xrt_render_var(m_ctx, &p, image.data(), variance.data(), &m_stats);
    if (rc != XRT_OK) fail(rc, std::string("xrt_render_var: ") + xrt_last_error(m_ctx));
}

void HipRenderer::beginProgressive(const Scene& scene, Sampler::SamplerType, const Image& image, bool variance) const {
    xrt_render_params p;
    if (!renderInputs(scene, image, p)) return;
    const int rc = xrt_progressive_begin(m_ctx, &p, variance ? XRT_PROGRESSIVE_VARIANCE : 0u);
    if (rc != XRT_OK) fail(rc, std::string("xrt_progressive_begin: ") + xrt_last_error(m_ctx));
}

void HipRenderer::addSamples(uint32_t n) const {
    if (context() != XRT_OK) return;
    const int rc = xrt_progressive_add(m_ctx, n, &m_stats);
    if (rc != XRT_OK) fail(rc, std::string("xrt_progressive_add: ") + xrt_last_error(m_ctx));
}

void HipRenderer::progressiveFrame(Image& image, std::vector<float>* variance) const {
    if (context() != XRT_OK) return;
    if (variance) variance->assign((size_t)image.getWidth() * image.getHeight(), 0.0f);
    const int rc = xrt_progressive_frame(m_ctx, image.data(), variance ? variance->data() : nullptr);
    if (rc != XRT_OK) fail(rc, std::string("xrt_progressive_frame: ") + xrt_last_error(m_ctx));
}

uint32_t HipRenderer::samplesDone() const {
    xrt_progressive_state s{};
    return m_ctx && xrt_progressive_query(m_ctx, &s) == XRT_OK ? s.spp_done : 0u;
}

void HipRenderer::endProgressive() const {
    if (m_ctx) (void)xrt_progressive_end(m_ctx);
}

bool HipRenderer::renderInputs(const Scene& scene, const Image& image, xrt_render_params& p) const {
    auto fail = [&](int rc, const char* what) {
        m_status = rc;
        m_error = std::string(what) + ": " + (m_ctx ? xrt_last_error(m_ctx) : xrt_last_error(nullptr));
        std::fprintf(stderr, "[HipRenderer] %s\n", m_error.c_str());
        return false;
    };
    int rc = prepare(scene);
    if (rc != XRT_OK) return false;

    std::memset(&p, 0, sizeof(p));
    switch (integrator->kind()) {
        case Integrator::Kind::GI: p.integrator = XRT_INTEGRATOR_GI; break;
        case Integrator::Kind::Direct: p.integrator = XRT_INTEGRATOR_DIRECT; break;
        case Integrator::Kind::VolumePathTracing: p.integrator = XRT_INTEGRATOR_VPT; break;
        case Integrator::Kind::Indirect: p.integrator = XRT_INTEGRATOR_INDIRECT; break;
        case Integrator::Kind::Normal: p.integrator = XRT_INTEGRATOR_NORMAL; break;
        case Integrator::Kind::VolumePathTracingNEE: p.integrator = XRT_INTEGRATOR_VPT_NEE; break;
        case Integrator::Kind::Whitted: p.integrator = XRT_INTEGRATOR_WHITTED; break;
        case Integrator::Kind::Custom:
            return fail(XRT_ERR_UNSUPPORTED, "custom Integrator subclasses have no GPU form");
    }
    const HomogeneousMedium* hom = dynamic_cast<const HomogeneousMedium*>(scene.anyMedium());
    if ((p.integrator == XRT_INTEGRATOR_VPT || p.integrator == XRT_INTEGRATOR_VPT_NEE) && hom) {
        xrt_medium_desc md;
        std::memset(&md, 0, sizeof(md));
        md.kind = dynamic_cast<const HomogeneousMediumAchromatic*>(hom) ? XRT_MEDIUM_HOMOGENEOUS_ACHROMATIC
                  : dynamic_cast<const HomogeneousMediumNoMIS*>(hom)    ? XRT_MEDIUM_HOMOGENEOUS_NOMIS
                                                                        : XRT_MEDIUM_HOMOGENEOUS_MIS;
        for (int c = 0; c < 3; ++c) {
            md.bbox_min[c] = hom->bounds().pMin[c];
            md.bbox_max[c] = hom->bounds().pMax[c];
            md.absorption[c] = hom->sigmaA()[c];
            md.scattering[c] = hom->sigmaS()[c];
        }
        md.g = hom->g();
        if ((rc = xrt_set_medium(m_ctx, &md)) != XRT_OK) return fail(rc, "xrt_set_medium");
    } else if (p.integrator == XRT_INTEGRATOR_VPT || p.integrator == XRT_INTEGRATOR_VPT_NEE) {
        const HeterogeneousMedium* med = scene.medium();
        const DenseGrid* grid = med ? dynamic_cast<const DenseGrid*>(med->grid()) : nullptr;
        const SparseGrid* sparse = med ? dynamic_cast<const SparseGrid*>(med->grid()) : nullptr;
        if (!grid && !sparse)
            return fail(XRT_ERR_UNSUPPORTED, "VolumePathTracing needs a HeterogeneousMedium over a DenseGrid or SparseGrid");
        xrt_medium_desc md;
        std::memset(&md, 0, sizeof(md));
        md.nx = grid ? grid->nx() : sparse->nx(), md.ny = grid ? grid->ny() : sparse->ny();
        md.nz = grid ? grid->nz() : sparse->nz();
        const AABB b = med->grid()->getBounds();
        const Vec3f& origin = grid ? grid->origin() : sparse->origin();
        for (int c = 0; c < 3; ++c) {
            md.origin[c] = origin[c];
            md.bbox_min[c] = b.pMin[c];
            md.bbox_max[c] = b.pMax[c];
            md.absorption[c] = med->absorptionColor()[c];
            md.scattering[c] = med->scatteringColor()[c];
        }
        md.voxel_size = grid ? grid->voxelSize() : sparse->voxelSize();
        md.max_density = med->grid()->getMaxDensity();
        md.g = med->g();
        md.density_multiplier = med->densityMultiplier();
        if (grid) {
            md.density = grid->data().data();
            if ((rc = xrt_set_medium(m_ctx, &md)) != XRT_OK) return fail(rc, "xrt_set_medium");
        } else {   // leaf bricks (NanoVDB layout)
            const xrt_brick_grid bg{sparse->bricksX(), sparse->bricksY(), sparse->bricksZ(), sparse->table().data(),
                                    sparse->brickCount(), sparse->bricks().data()};
            if ((rc = xrt_set_medium_bricks(m_ctx, &md, &bg)) != XRT_OK) return fail(rc, "xrt_set_medium_bricks");
        }
    }
    p.max_depth = integrator->maxDepth();
    p.width = image.getWidth();
    p.height = image.getHeight();
    p.spp = n_samples;
    p.shard_index = 0;
    p.shard_count = 1;
    // the reference's Whitted loop runs over any Scene: take the BVH schedule when LDS is too small
    if (p.integrator == XRT_INTEGRATOR_WHITTED) p.flags |= XRT_FLAG_WHITTED_BVH;
    return true;
}
