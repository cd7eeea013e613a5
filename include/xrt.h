/*
 * xrt.h — C ABI of libxrt_hip.so, the MI355X (gfx950) path-tracing backend that sits
 * behind the reference's Renderer::render() (Src/renderer.h:15).
 *
 * The reference has no FFI: its plugin surface is the C++ virtual class
 *   virtual void Renderer::render(const Scene&, Sampler::SamplerType, Image&) const = 0;
 * (Src/renderer.h:8-20).  A renderer that replaces NormalRenderer / ParallelRenderer
 * (Src/renderer.cpp:8-27, 83-99) needs exactly four things from the caller's objects:
 *   - the scene's objects in Scene::m_objects iteration order (Src/scene.h:45, scene.cpp:190-211),
 *   - the area lights in Scene::m_areaLights order             (Src/scene.h:44, scene.cpp:166-188),
 *   - the pinhole camera (c2w, scale, aspect)                   (Src/camera.h:10-11,37-60),
 *   - the integrator kind and its max depth                     (Src/integrator.h:198-291,76-120,401-478),
 *   - for WhittedIntegrator the delta lights in Scene::m_deltaLights order (Src/scene.cpp:161-163),
 * and it must fill an Image of W*H float3 in place with the per-pixel sample mean
 * (Src/renderer.cpp:29-81,98; Src/image.h:46-78).  Every entry point below maps onto
 * one of those steps.  The C++ HipRenderer (include/xrt/renderer.h) is the
 * reference-side binding; INTEGRATION.md shows it.
 *
 * Conventions: plain C types only; the caller owns all host memory and the library
 * copies what it needs; status 0 = XRT_OK, negative = error (xrt_last_error gives
 * text); no C++ exception crosses this boundary.  A context is used by one host thread.
 * Multi-GPU, two ways: one process per GPU with one context each, rendering row shards
 * (shard_index / shard_count) and reducing the framebuffers over RCCL (the bench); or one
 * process with one context over several GPUs (xrt_create_multi), which shards and
 * assembles the frame itself (ParallelRenderer over the node, Src/renderer.cpp:83-99).
 */
#ifndef XRT_H
#define XRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XRT_ABI_VERSION 14

/* ---- status codes ---------------------------------------------------------------- */
enum {
    XRT_OK = 0,
    XRT_ERR_INVALID = -1,     /* bad argument / inconsistent scene */
    XRT_ERR_HIP = -2,         /* HIP runtime error (no GPU, launch failure, fault) */
    XRT_ERR_STATE = -3,       /* call order: e.g. render before upload */
    XRT_ERR_OOM = -4,         /* device allocation failed */
    XRT_ERR_UNSUPPORTED = -5, /* feature outside the supported set */
    XRT_ERR_IO = -6           /* file could not be read / parsed (Scene::loadObj exit(1)) */
};

/* ---- scene description (flattened Scene) ------------------------------------------ */
enum { XRT_OBJ_MESH = 0, XRT_OBJ_SPHERE = 1, XRT_OBJ_BOX = 2 };
/* XRT_LIGHT_SPHERE: SphereLight::sample's default (cone) branch (Src/light.h:157-197);
 * XRT_LIGHT_SPHERE_AREA: the same light built with AREA_SAMPLING (Src/light.h:131-135,185-191:
 * a uniform point on the sphere, UniformSampleSphere Src/light.cpp:99-105, pdf 2 tmax^3/|d.n|) */
enum { XRT_LIGHT_QUAD = 0, XRT_LIGHT_TRIANGLE = 1, XRT_LIGHT_SPHERE = 2, XRT_LIGHT_SPHERE_AREA = 3 };
/* XRT_MAT_METAL / XRT_MAT_GLASS: Object::materialType() returning MaterialType::Metals / Glass
 * (Src/geometry.h:703), the mirror and dielectric branches of WhittedIntegrator
 * (Src/integrator.h:344-381).  They are valid only under XRT_INTEGRATOR_WHITTED: every other
 * integrator would call the material's own BxDF there, which the backend cannot know, and
 * returns XRT_ERR_UNSUPPORTED for a scene that holds one. */
enum { XRT_MAT_NONE = 0, XRT_MAT_LAMBERT = 1, XRT_MAT_METAL = 2, XRT_MAT_GLASS = 3 };

/* One Object (Src/primitive.h:40-95) in Scene::m_objects iteration order. */
typedef struct {
    int32_t kind;       /* XRT_OBJ_*                                                     */
    int32_t first;      /* first primitive in the kind's array (tris / spheres / boxes)  */
    int32_t count;      /* number of primitives (mesh: triangles; sphere/box: 1)         */
    int32_t material;   /* XRT_MAT_* (Object::m_material != nullptr)                     */
    float albedo[3];    /* Lambert::m_albedo (Src/material.h:76)                         */
    int32_t light;      /* index into lights[] or -1 (Object::m_areaLight)               */
    int32_t medium;     /* 0 = the scene medium, -1 = none (Object::m_medium)            */
} xrt_object;

/* One AreaLight (Src/light.h:54-210) in Scene::m_areaLights order, world space. */
typedef struct {
    int32_t kind;       /* XRT_LIGHT_*                                                   */
    float v0[3];        /* quad / triangle vertices after multVecMatrix(l2w)             */
    float v1[3];
    float v2[3];
    float center[3];    /* sphere light                                                  */
    float radius;
    float Le[3];        /* AreaLight::Le_                                                */
} xrt_light;

typedef struct {
    uint32_t n_objects;
    const xrt_object* objects;
    uint32_t n_tris;
    const float* tri_v;      /* [n_tris][3][3] vertices (Primitive::m_vertices)       */
    const float* tri_n;      /* [n_tris][3][3] vertex normals (Primitive::m_normals)  */
    uint32_t n_spheres;
    const float* spheres;    /* [n_spheres][4] center.xyz, radius                      */
    uint32_t n_boxes;
    const float* boxes;      /* [n_boxes][6] pMin.xyz, pMax.xyz (AABB)                 */
    uint32_t n_lights;
    const xrt_light* lights;
} xrt_scene_desc;

/* One DeltaLight (Src/light.h:11-49) in Scene::m_deltaLights order (a std::vector: push-back
 * order, Src/scene.cpp:161-163), world space.  Only WhittedIntegrator reads them. */
enum { XRT_DLIGHT_POINT = 0, XRT_DLIGHT_DISTANT = 1 };
typedef struct {
    int32_t kind;       /* XRT_DLIGHT_*                                                   */
    float pos[3];       /* PointLight::pos: multVecMatrix(Vec3f(0)) (Src/light.cpp:115-118) */
    float dir[3];       /* DistantLight::dir: normalize(multDirMatrix((0,0,-1))) (:130-134) */
    float color[3];     /* DeltaLight::color                                              */
    float intensity;    /* DeltaLight::intensity                                          */
} xrt_delta_light;
#define XRT_MAX_DELTA_LIGHTS 8   /* most delta lights a context takes */

/* The scene medium.  kind XRT_MEDIUM_HETEROGENEOUS: HeterogeneousMedium over a dense
 * density grid standing in for DensityGrid (Src/grid.h:9-15): OpenVDB
 * BoxSampler::wsSample semantics — world -> index by (p - origin) / voxel_size, voxel
 * centres at integer index coordinates, trilinear, background 0 outside the data.
 * The homogeneous kinds (Src/medium.h:122-277) use absorption / scattering as sigma_a /
 * sigma_s (Achromatic: channel 0 of each), bbox as the medium box and g; the grid fields
 * (nx..voxel_size, max_density, density_multiplier) are ignored and density may be NULL. */
enum {
    XRT_MEDIUM_HETEROGENEOUS = 0,          /* HeterogeneousMedium (delta / ratio tracking)  */
    XRT_MEDIUM_HOMOGENEOUS_MIS = 1,        /* HomogeneousMediumMIS (Src/medium.h:148-192)   */
    XRT_MEDIUM_HOMOGENEOUS_ACHROMATIC = 2, /* HomogeneousMediumAchromatic (:195-231)        */
    XRT_MEDIUM_HOMOGENEOUS_NOMIS = 3       /* HomogeneousMediumNoMIS (:234-277)             */
};
typedef struct {
    uint32_t nx, ny, nz;
    const float* density;    /* [nz][ny][nx]                                           */
    float origin[3];         /* world position of index (0,0,0)                         */
    float voxel_size;
    float bbox_min[3];       /* DensityGrid::getBounds() (world)                        */
    float bbox_max[3];
    float max_density;       /* DensityGrid::getMaxDensity()                            */
    float g;                 /* HenyeyGreenstein g                                      */
    float absorption[3];     /* HeterogeneousMedium::absorptionColor                    */
    float scattering[3];     /* HeterogeneousMedium::scatteringColor                    */
    float density_multiplier;
    int32_t kind;            /* XRT_MEDIUM_* (0 when zero-initialised: heterogeneous)   */
} xrt_medium_desc;

/* ---- render parameters --------------------------------------------------------------- */
enum {
    XRT_INTEGRATOR_GI = 0,        /* GIIntegrator(maxDepth)            Src/integrator.h:198-291 */
    XRT_INTEGRATOR_DIRECT = 1,    /* DirectIntegrator                  Src/integrator.h:76-120  */
    XRT_INTEGRATOR_VPT = 2,       /* VolumePathTracing(maxDepth)       Src/integrator.h:401-478 */
    XRT_INTEGRATOR_INDIRECT = 3,  /* IndirectIntegrator(maxDepth)      Src/integrator.h:122-190 */
    XRT_INTEGRATOR_NORMAL = 4,    /* NormalIntegrator (shading normal) Src/integrator.h:22-74   */
    XRT_INTEGRATOR_VPT_NEE = 5,   /* VolumePathTracingNEE(maxDepth)    Src/integrator.h:481-636 */
    XRT_INTEGRATOR_WHITTED = 6    /* WhittedIntegrator(maxDepth)       Src/integrator.h:294-398 */
};
/* WhittedIntegrator limits.  By default it runs only over scenes that fit the LDS-resident
 * scene carve (the scenes the fused and pixel schedules serve: triangle, sphere and mixed
 * scenes up to 64 KiB); larger (two-level) scenes return XRT_ERR_UNSUPPORTED.  With
 * XRT_FLAG_WHITTED_BVH a triangle scene beyond LDS renders through its triangle BVH
 * (XRT_SCHED_WHITTED_BVH); large sphere-only and mixed scenes, which have no triangle BVH,
 * still return XRT_ERR_UNSUPPORTED.  A glass hit pushes two
 * rays, so a scene with a glass object has a ray tree of up to 2^(max_depth + 1) leaves and
 * max_depth above XRT_WHITTED_MAX_DEPTH returns XRT_ERR_UNSUPPORTED; scenes without glass are
 * chains and take any max_depth.  The schedule flags XRT_FLAG_WAVEFRONT, NO_PIXEL, NO_MERGED,
 * NO_SPEC, NO_GROUP and DEEP_* have no effect on it. */
#define XRT_WHITTED_MAX_DEPTH 4
enum {
    XRT_FLAG_TIMING = 1u,      /* time every kernel with HIP events (xrt_stats.kernel_ms)     */
    XRT_FLAG_WAVEFRONT = 2u,   /* force the multi-pass schedule (k_shade + k_trace) even when
                                  the scene fits the fused LDS-resident schedule (k_step)     */
    XRT_FLAG_NO_MERGED = 4u,   /* triangle scenes: per-segment cooperative traces (k_step_tri)
                                  instead of the merged shadow + extension traces             */
    XRT_FLAG_NO_GROUP = 8u,    /* merged schedule with 16/32 slots per wave: spread the traces
                                  over idle lanes (pair passes) instead of 4/2-lane groups    */
    XRT_FLAG_DEEP_SINGLE = 32u, /* two-level traces: walk the BVH with one lane per queued ray  */
    XRT_FLAG_DEEP_QUAD = 64u,   /* ... with four lanes per ray (the default); results never
                                   depend on either                                            */
    XRT_FLAG_NO_PIXEL = 128u,   /* Direct / Normal: the per-slot fused schedule (k_step) instead
                                   of pixel-parallel sample chains (k_pixel); same results     */
    XRT_FLAG_NO_SPEC = 256u,    /* GI, one light, small all-Lambert triangle scenes: the merged schedule's
                                   16-slot launches start every sample beside its predecessor's
                                   last trace (k_step_spec, the default); this flag keeps them on
                                   k_step_merged — same results                                */
    XRT_FLAG_WHITTED_BVH = 512u, /* Whitted may fall back to the global-memory BVH schedule when
                                   the scene does not fit LDS (k_whitted_bvh: triangle scenes
                                   with one big mesh or many, XRT_SCHED_WHITTED_BVH); a scene
                                   that fits LDS renders exactly as without the flag           */
    XRT_FLAG_NO_OVERLAP = 1024u, /* merged schedule: one step launch per round on the context's
                                   stream, instead of one per partition group on streams of their
                                   own (the default while whole waves run, XRT_STEP_GROUPS in
                                   tuning.h); same results                                     */
    XRT_FLAG_INTERLEAVE = 2048u, /* merged schedule: slot s renders pixel s * A mod n of the shard's
                                   n pixels, so every wave of 64 slots samples the whole shard
                                   (csrc/slot_map.h).  By default a merged render of a large shard
                                   does (XRT_SLOT_INTERLEAVE in tuning.h); this flag makes a merged
                                   render of any size do it.  No effect on the other schedules;
                                   same results                                                 */
    XRT_FLAG_NO_INTERLEAVE = 4096u, /* ... and this one keeps every render on the row-major map
                                   (slot s = pixel s); it wins over XRT_FLAG_INTERLEAVE          */
    XRT_FLAG_VAR_FUSED = 8192u, /* xrt_render_var / xrt_render_var_device only: the path integrators
                                   keep the fused or merged schedule instead of the wavefront (see
                                   there); every other entry point ignores it; same results      */
    XRT_FLAG_CHUNKS = 16384u,   /* merged schedule, one-level scenes: while whole waves run, the live
                                   slots stay in chunks of 256 that one block per launch owns and
                                   steps for several rounds (k_step_merged_chunks, csrc/step_chunks.h)
                                   instead of one launch per round and partition group.  By default
                                   a large interleaved render of many samples does, when the caller
                                   sets neither visits_per_launch nor slots_per_wave; this flag makes
                                   every such render that starts at 64 slots per wave do it.
                                   XRT_FLAG_NO_OVERLAP keeps its meaning (the grouped rounds before
                                   and after the phase) and does not disable chunks; same results */
    XRT_FLAG_NO_CHUNKS = 32768u, /* ... and this one keeps every render on the grouped schedule; it
                                   wins over XRT_FLAG_CHUNKS                                      */
    XRT_FLAG_ACCUMULATE = 16u  /* Renderer::render's in-place contract (Src/renderer.cpp:75,98):
                                  each owned pixel starts from the value already in the output
                                  buffer (Image::addPixel adds to it in sample order), then
                                  /= spp; pixels of other shards are left untouched.  Without
                                  the flag the buffer is overwritten (zeros outside the shard). */
};

typedef struct {
    int32_t integrator;      /* XRT_INTEGRATOR_*                                        */
    uint32_t max_depth;      /* GIIntegrator / VolumePathTracing m_maxDepth             */
    uint32_t width, height;  /* Image size                                              */
    uint32_t spp;            /* NormalRenderer::n_samples                               */
    uint32_t shard_index;    /* this rank owns image rows y with y % shard_count == idx */
    uint32_t shard_count;    /* 1 = whole image                                         */
    uint32_t flags;          /* XRT_FLAG_*                                              */
    /* launch geometry of the merged schedule; 0 = chosen by the library from the shard's
     * slot count.  Results never depend on these (tests render every layout). */
    uint32_t slots_per_wave;    /* 0, 4, 8, 16, 32 or 64 path slots per 64-lane wave     */
    uint32_t visits_per_launch; /* 0 or 1..128 path segments per slot per step launch    */
} xrt_render_params;

/* kernel families timed in xrt_stats: XRT_K_TRACE is the wavefront trace (for two-level
 * scenes its phase A, the small objects), XRT_K_DEEP the BVH walk of the rays phase A queued */
enum {
    XRT_K_SEED = 0, XRT_K_TRACE = 1, XRT_K_SHADE = 2, XRT_K_FINISH = 3, XRT_K_STEP = 4, XRT_K_REFILL = 5,
    XRT_K_DEEP = 6, XRT_K_COUNT = 7
};

/* device schedules: multi-pass wavefront (k_shade + k_trace), fused per-slot k_step with
 * the scene in LDS, its triangle-scene form with cooperative (ray, triangle) traces, that
 * form with one merged trace (shadow rays + next extension ray) per segment, the merged
 * form for two-level scenes (small objects in LDS, a big mesh's BVH walked by the wave), and
 * for the one-trace integrators (Direct, Normal) pixel-parallel sample chains: one wave per
 * pixel evaluates 64 candidate samples at once and keeps those on the pixel's chain (k_pixel;
 * timed as XRT_K_STEP) */
enum {
    XRT_SCHED_WAVEFRONT = 0, XRT_SCHED_STEP = 1, XRT_SCHED_STEP_TRI = 2, XRT_SCHED_STEP_MERGED = 3,
    XRT_SCHED_STEP_BVH = 4, XRT_SCHED_PIXEL = 5,
    XRT_SCHED_WHITTED = 6,  /* WhittedIntegrator: one wave per pixel, one lane per sample, the whole
                               ray tree of a sample in its lane (k_whitted; timed as XRT_K_STEP) */
    XRT_SCHED_WHITTED_BVH = 7,  /* the same loop over a triangle scene beyond LDS, its traces through
                                   the triangle BVH (k_whitted_bvh, XRT_FLAG_WHITTED_BVH)           */
    XRT_SCHED_AOV = 8           /* xrt_render_aov: one wave per pixel, one lane per sample, one
                                   Scene::intersect each (k_aov / k_aov_bvh; timed as XRT_K_STEP)   */
};

typedef struct {
    double wall_ms;              /* host wall clock of the render call (upload excluded) */
    double kernel_ms[XRT_K_COUNT];   /* summed HIP-event time per kernel (XRT_FLAG_TIMING) */
    uint64_t launches[XRT_K_COUNT];  /* launches per kernel                                */
    /* While the merged schedule's step launches run in partition groups, a round is one launch
     * per group, each on its group's stream: launches[XRT_K_STEP] and layout_launches count every
     * one of them, `iterations` the rounds.  Their times overlap, so per-launch events would sum to
     * the groups' number times the wall time: the grouped rounds are timed as one span, from the
     * fork off the context's stream to the join back into it, and that span is what
     * kernel_ms[XRT_K_STEP] gets.  kernel_ms / launches stays the time one launch costs the frame. */
    uint64_t samples;            /* pixels * spp rendered by this shard                    */
    uint64_t segments;           /* Scene::intersect calls (extension rays traced)         */
    uint64_t shadow_rays;        /* Scene::occluded calls                                  */
    uint64_t draws;              /* RNG draws (Sampler::getNext1D)                         */
    uint64_t rejected;           /* samples dropped by the NaN/Inf/negative check          */
    uint64_t iterations;         /* trace+shade pass pairs, or k_step rounds               */
    uint64_t path_slots;         /* slots in flight (pixels of this shard)                 */
    uint64_t schedule;           /* XRT_SCHED_* the render ran                             */
    uint64_t stalled;            /* paths stopped by the VPT no-progress guard             */
    /* launch geometry the render ran with (merged schedules; 0 otherwise) */
    uint32_t slots_per_wave;     /* path slots per wave of the first step launch            */
    uint32_t group_lanes;        /* lanes sharing one slot's traces (1 = pair passes)      */
    uint32_t partitions;         /* live-list partitions                                   */
    uint32_t visits_per_launch;  /* path segments per slot per step launch                 */
    uint64_t rng_twists;         /* mt19937 blocks generated (624 words each) over all slots,
                                    including each slot's first: rng_twists - path_slots is
                                    the number of ring refills done while paths were live  */
    uint64_t layout_launches[5]; /* merged schedules: step launches per slots-per-wave layout
                                    64, 32, 16, 8, 4 (the layout is re-chosen every launch
                                    from the live count)                                   */
    /* pixel-parallel chains (XRT_SCHED_PIXEL): which of k_pixel's paths ran */
    uint64_t pix_windows;        /* candidate windows evaluated (64 offsets each)           */
    uint64_t pix_stride4;        /* ... of them at stride 4 (after a window of surface hits) */
    uint64_t pix_frustum;        /* pixels whose camera rays tested a camera-frustum list   */
    uint64_t pix_frustum_overflow; /* pixels whose frustum list overflowed (BVH walks)      */
    uint64_t pix_shadow_list;    /* pixels whose shadow rays tested an occluder list        */
    uint64_t pix_shadow_overflow;  /* pixels whose occluder list overflowed (BVH walks)     */
    uint64_t pix_flushes;        /* deferred-shading queue flushes                          */
    uint64_t spec_launches;      /* merged schedule: step launches with speculative starts  */
    /* WhittedIntegrator (XRT_SCHED_WHITTED); segments = Scene::intersect calls, shadow_rays =
     * Scene::occluded calls, draws = 2 * samples there */
    uint64_t whit_rays;          /* rays popped from the queue (depth-overflow pops included) */
    uint64_t whit_depth_cut;     /* ... of them with depth > max_depth                       */
    uint64_t whit_refract;       /* glass hits with kr < 1 (a refracted and a reflected ray) */
    uint64_t whit_tir;           /* glass hits with kr >= 1 (total internal reflection)      */
} xrt_stats;

/* ---- context ----------------------------------------------------------------------- */
typedef struct xrt_ctx xrt_ctx;

int  xrt_abi_version(void);
/* device = HIP device ordinal (one process per GPU: LOCAL_RANK) */
int  xrt_create(int device, xrt_ctx** out);
/* One context over n_devices GPUs (HIP ordinals; a device may be listed twice, e.g. to
 * exercise the multi-GPU path on one GPU).  Every call fans out to all of them; a render
 * gives device i the interleaved rows y % (n * shard_count) == shard_index + shard_count * i
 * (one host thread and HIP stream per device, concurrently) and assembles the frame on
 * devices[0] with one strided peer copy per device — bit-identical to a one-GPU render.
 * xrt_render_device* take a device pointer on devices[0]. */
int  xrt_create_multi(const int* devices, int n_devices, xrt_ctx** out);
int  xrt_device_count(const xrt_ctx* ctx);   /* GPUs a context renders on */
void xrt_destroy(xrt_ctx* ctx);
const char* xrt_last_error(const xrt_ctx* ctx);   /* ctx may be NULL (create failure) */

/* Where results are bit-identical to the reference.  The acceleration structures an upload
 * builds (padded object boxes, the plane cull, the padded boxes of the triangle and sphere
 * BVHs) only skip primitives the reference's in-order scan would have rejected, as long as
 * the scene's vertices and the origins of the rays traced — the camera's position — lie
 * within XRT_EXACT_DIAGONALS scene diagonals of the world origin resp. of the scene; a scene
 * of triangle meshes only: within XRT_EXACT_DIAGONALS_TRI.  The margins of those boxes are
 * relative to the scene's size, while the float error of a hit grows with the distance of
 * the ray origin and of the scene from the world origin: beyond the domain a hit within
 * float error of an object's silhouette, or whose distance the reference's own arithmetic
 * no longer resolves, may be reported as a miss or as the hit behind it.  Both numbers lie
 * two octaves below the first failure measured by tests/test_adversarial_rays.py (DESIGN.md
 * section 3, "Where the culls are exact"). */
#define XRT_EXACT_DIAGONALS 1.0f
#define XRT_EXACT_DIAGONALS_TRI 16.0f
int  xrt_upload_scene(xrt_ctx* ctx, const xrt_scene_desc* scene);
/* Camera::camera2world (row-major, row-vector convention, Src/geometry.h:486-498),
 * PinholeCamera::scale = tan(0.5*deg2rad(FOV)) and aspect_ratio (Src/camera.h:37-47).
 * The eye (c2w's last row) is the origin of every camera ray: renders are bit-identical to
 * the reference's while it lies within XRT_EXACT_DIAGONALS (XRT_EXACT_DIAGONALS_TRI) scene
 * diagonals of the scene, however narrow the field of view (see xrt_upload_scene). */
int  xrt_set_camera(xrt_ctx* ctx, const float c2w[16], float scale, float aspect);
int  xrt_set_medium(xrt_ctx* ctx, const xrt_medium_desc* medium);
/* The delta lights of the scene (Scene::getDeltaLights(), Src/scene.h), in order; n = 0 clears
 * them, n > XRT_MAX_DELTA_LIGHTS returns XRT_ERR_UNSUPPORTED.  They belong to the context, not
 * to the uploaded scene: xrt_upload_scene does not clear them.  On a multi-device context the
 * call fans out like every other. */
int  xrt_set_delta_lights(xrt_ctx* ctx, const xrt_delta_light* lights, uint32_t n);
/* Sparse heterogeneous density in leaf bricks (the layout NanoVDB / OpenVDB give a grid:
 * 8^3-voxel leaves, Src/examples/nanovdb_convert.cpp, Src/grid.h:22-83).  The grid's
 * index space [0, nx) x [0, ny) x [0, nz) is cut into XRT_BRICK^3 bricks;
 * table[(bz * nby + by) * nbx + bx] is the brick's index in `bricks` or -1 (inactive:
 * background 0, as OpenVDB's BoxSampler reads it).  bricks[b] holds XRT_BRICK^3 floats in
 * [z][y][x] order.  Sampling is the same trilinear BoxSampler as the dense grid, so a brick
 * grid renders bit-identically to the dense grid it was cut from.  medium->density is
 * ignored; every other field of xrt_medium_desc keeps its meaning. */
#define XRT_BRICK 8
typedef struct {
    uint32_t nbx, nby, nbz;      /* bricks per axis: ceil(n / XRT_BRICK)                    */
    const int32_t* table;        /* [nbz][nby][nbx] brick index or -1                        */
    uint32_t n_bricks;
    const float* bricks;         /* [n_bricks][XRT_BRICK^3]                                  */
} xrt_brick_grid;
int  xrt_set_medium_bricks(xrt_ctx* ctx, const xrt_medium_desc* medium, const xrt_brick_grid* grid);

/* Render into caller-owned HOST memory rgb_out[height][width][3] (Image::pixels order
 * j + width*i).  Pixels outside this shard are written as 0.  Blocks until done. */
int  xrt_render(xrt_ctx* ctx, const xrt_render_params* p, float* rgb_out, xrt_stats* st);
/* Same, writing into a DEVICE pointer on this context's GPU (e.g. a torch tensor), so a
 * multi-GPU caller can reduce framebuffers over RCCL without a host round trip.
 * Ordering: the render starts only after all work previously queued on the device has
 * finished (a device-wide wait), so it never overwrites d_rgb_out while a collective or
 * copy issued by the caller still reads it.  Returns after the image is complete. */
int  xrt_render_device(xrt_ctx* ctx, const xrt_render_params* p, float* d_rgb_out, xrt_stats* st);
/* As xrt_render_device, but waits only for the work queued so far on `hip_stream` (a
 * hipStream_t of this context's GPU, e.g. torch.cuda.current_stream().cuda_stream; NULL =
 * the legacy default stream) before touching d_rgb_out. */
int  xrt_render_device_after(xrt_ctx* ctx, const xrt_render_params* p, float* d_rgb_out, void* hip_stream,
                             xrt_stats* st);

/* ---- a render with its per-pixel sample variance ---------------------------------------- */
/* The frame of xrt_render and, beside it, the variance of each pixel's mean luminance: the
 * plane xrt_denoise_var reads as `variance`.
 *   rgb_out      [H][W][3]  exactly xrt_render's frame for the same p, bit for bit, the sign of
 *                           a zero included
 *   variance_out [H][W]     from the pixel's own samples, in IEEE float32, one rounding per
 *                           operation, no FMA:
 *       lum(r) = (0.2126f r.x + 0.7152f r.y) + 0.0722f r.z
 *       s1 = s2 = +0
 *       for the samples k = 0 .. spp - 1 in sample order, each sample r that Image::addPixel
 *       accepts (not NaN / Inf / negative: the test the frame uses)
 *           l  = lum(r)
 *           s1 = s1 + l
 *           s2 = s2 + l * l
 *       n        = (float)spp
 *       mean     = s1 / n
 *       v        = s2 / n - mean * mean
 *       v        = v > 0 ? v : +0
 *       variance = v / (float)(spp - 1)
 *     A rejected sample adds nothing and n stays spp, as for the frame.
 * Pixels outside the shard are +0 in both planes.
 * Refusals: XRT_ERR_INVALID for a NULL ctx, p, rgb_out or variance_out and for spp < 2 (one sample
 * has no variance); XRT_ERR_UNSUPPORTED with XRT_FLAG_ACCUMULATE (the moments of the earlier
 * calls' samples are unknown); and everything xrt_render refuses, the same way.
 * Schedule: the six path integrators always run the wavefront schedule (XRT_SCHED_WAVEFRONT),
 * WhittedIntegrator XRT_SCHED_WHITTED / XRT_SCHED_WHITTED_BVH as in xrt_render; the other schedule
 * flags, slots_per_wave and visits_per_launch are checked as xrt_render checks them and have no
 * effect.  XRT_FLAG_TIMING works.  Every xrt_stats field is what xrt_render reports for the same
 * p with XRT_FLAG_WAVEFRONT set (the plane's kernel runs and is timed under XRT_K_FINISH).
 * With XRT_FLAG_VAR_FUSED the six path integrators instead run the schedule xrt_render chooses for
 * p with XRT_FLAG_NO_SPEC | XRT_FLAG_NO_PIXEL added (the speculative and the pixel-parallel kernels
 * sum no moments): every other schedule flag, slots_per_wave and visits_per_launch then count as
 * they do for xrt_render.  The frame and the plane are bit for bit those of the call without the
 * flag — the arithmetic above is the whole contract — and every xrt_stats field is what xrt_render
 * reports for p | XRT_FLAG_NO_SPEC | XRT_FLAG_NO_PIXEL; the plane's kernel stays under
 * XRT_K_FINISH.  Where that schedule is the wavefront (the scene does not fit the fused schedule,
 * or XRT_FLAG_WAVEFRONT is set) and for WhittedIntegrator the call is the one without the flag.
 * The refusals do not change.
 * A multi-device context shards rows as for a render and assembles both planes on devices[0].
 * After the call the context's last framebuffer — what xrt_tonemap and the filters read for a
 * NULL colour — is this frame, for the device entry point too. */
/* into caller-owned HOST memory; blocks until done */
int  xrt_render_var(xrt_ctx* ctx, const xrt_render_params* p, float* rgb_out, float* variance_out, xrt_stats* st);
/* into DEVICE pointers on this context's GPU (devices[0]); ordering as xrt_render_device_after:
 * waits only for the work queued so far on hip_stream (NULL = the legacy default stream) */
int  xrt_render_var_device(xrt_ctx* ctx, const xrt_render_params* p, float* d_rgb_out, float* d_variance_out,
                           void* hip_stream, xrt_stats* st);

/* ---- progressive rendering: add samples to a frame --------------------------------------- */
/* A session renders a frame in passes: begin seeds the pixels' streams, every add renders spp more
 * samples of each pixel from where its stream stands, and frame gives the mean of the samples so far.
 * A pixel's samples are one sequential mt19937 stream, so passes of n1, n2, ... samples give, bit for
 * bit, the frame, the variance plane and the path counters of one xrt_render / xrt_render_var at
 * n1 + n2 + ... samples: 16 spp on screen, then 64, then 1024 cost 1024 samples, not 1104.
 *
 * xrt_progressive_begin checks p exactly as xrt_render does (p->spp is ignored), fixes the slot ->
 * pixel map and the partitions, seeds every slot and zeroes a context-owned accumulator; it renders
 * nothing.  options: XRT_PROGRESSIVE_VARIANCE also sums the luminance moments of xrt_render_var.
 *   Schedule: the one xrt_render chooses for p->flags | XRT_FLAG_NO_SPEC | XRT_FLAG_NO_PIXEL; with the
 *   variance option the one xrt_render_var chooses under XRT_FLAG_VAR_FUSED for the same flags.  The
 *   pixels no camera ray can hit are traced like the others (no retirement before the path loop).
 *   Speculative sample starts, pixel-parallel chains and that retirement are not part of a session
 *   yet: their kernels keep no resumable state per slot.
 *   Refusals: everything xrt_render refuses, the same way; XRT_ERR_UNSUPPORTED for WhittedIntegrator
 *   (its kernels never write a stream position back), for XRT_FLAG_ACCUMULATE and for a multi-device
 *   context — row shards (shard_index / shard_count) work, so one process per GPU can run sessions.
 *   A second begin replaces the open session.
 * xrt_progressive_add renders spp more samples of every owned pixel into the accumulator and returns
 * when they are done.  XRT_ERR_INVALID for spp == 0, without an open session, and when the session's
 * sample count would overflow uint32_t.  Of *st, samples, segments, shadow_rays, draws, rejected and
 * stalled are the session's so far — those of one render of spp_done samples at the session's flags —
 * and schedule, iterations, launches, kernel_ms, wall_ms, the layout fields and rng_twists are this
 * call's (the kernel that resumes the slots counts under XRT_K_SEED).
 * xrt_progressive_frame: rgb_out[pixel] = accumulator[pixel] / (float)spp_done for the owned pixels,
 * +0 elsewhere; variance_out (may be NULL) is xrt_render_var's arithmetic with n = spp_done.  The
 * accumulator stays undivided: the call can be repeated and does not disturb the session.
 * XRT_ERR_INVALID before the first add, for variance_out without the variance option and for
 * variance_out at spp_done < 2.  Afterwards the context's last framebuffer — what xrt_tonemap and the
 * filters read for a NULL colour — is this frame.  The device entry point orders itself as
 * xrt_render_var_device does.
 * A session ends with xrt_progressive_end, with xrt_upload_scene, xrt_set_camera, xrt_set_medium*,
 * xrt_set_delta_lights, with every render entry point (xrt_render*, xrt_render_var*,
 * xrt_render_aov*) and with xrt_test_chunk_plan: afterwards add and frame return XRT_ERR_INVALID and
 * query gives active = 0.  xrt_denoise*, xrt_tonemap, xrt_query and xrt_last_error do not end it:
 * add, frame, denoise, add is the intended loop. */
enum { XRT_PROGRESSIVE_VARIANCE = 1u };   /* also sum the luminance moments of xrt_render_var */
typedef struct {
    uint32_t active;         /* 1 while a session is open on the context */
    uint32_t spp_done;       /* samples per pixel accumulated so far */
    uint32_t passes;         /* xrt_progressive_add calls that completed */
    uint32_t resume_twists;  /* slots whose ring the last add's resume had to twist */
    uint64_t path_slots;
} xrt_progressive_state;
int  xrt_progressive_begin(xrt_ctx* ctx, const xrt_render_params* p, uint32_t options);
int  xrt_progressive_add(xrt_ctx* ctx, uint32_t spp, xrt_stats* st);
/* into caller-owned HOST memory */
int  xrt_progressive_frame(xrt_ctx* ctx, float* rgb_out, float* variance_out);
/* into DEVICE pointers on this context's GPU */
int  xrt_progressive_frame_device(xrt_ctx* ctx, float* d_rgb_out, float* d_variance_out, void* hip_stream);
int  xrt_progressive_query(const xrt_ctx* ctx, xrt_progressive_state* out);
int  xrt_progressive_end(xrt_ctx* ctx);

/* ---- first-hit guide buffers (AOVs) --------------------------------------------------- */
/* Per-pixel guide planes for a denoiser or compositor, taken through the render's own camera
 * rays: sample k of pixel (row i, col j) takes words 2k, 2k + 1 of the pixel's stream (seed
 * j + width * i) as its jitter and builds PinholeCamera::sampleRay (Src/camera.h:49-60) as
 * every schedule does — bit for bit the camera rays of WhittedIntegrator and NormalIntegrator
 * at the same spp (for the other integrators sample 0 is the same ray).  Each sample is one
 * Scene::intersect and gives
 *   albedo [H][W][3]  Lambert: xrt_object.albedo as uploaded; Metal / Glass: (1, 1, 1);
 *                     XRT_MAT_NONE (emitters, medium boxes): (0, 0, 0)
 *   normal [H][W][3]  SurfaceInfo::ns as Scene::intersect leaves it
 *   depth  [H][W]     IntersectInfo::t
 *   alpha  [H][W]     1
 *   object [H][W]     int32: the object index (iteration order) of SAMPLE 0 only, -1 on a miss
 * A miss gives 0 in every float channel.  Every float channel starts at +0.0f, takes each
 * sample's value in sample order (a miss adds +0.0f) and is divided once by (float)spp; there
 * is no NaN / Inf / negative rejection.  Mean depth over the hits is depth / alpha (the
 * caller's division).  Pixels outside the shard are written 0 (object: -1).
 * A NULL member is a plane that is not wanted: it is neither computed into nor copied; all
 * five NULL returns XRT_ERR_INVALID.  width, height, spp (> 0), shard_index, shard_count and
 * XRT_FLAG_TIMING mean what they mean for xrt_render; integrator and max_depth are ignored
 * (metal and glass objects are accepted), the schedule flags have no effect, and
 * XRT_FLAG_ACCUMULATE returns XRT_ERR_UNSUPPORTED.  Scenes: those that fit the LDS-resident
 * scene carve, and triangle scenes beyond it through their triangle BVH (no flag needed);
 * large sphere-only and mixed scenes return XRT_ERR_UNSUPPORTED, as for WhittedIntegrator.
 * xrt_stats: samples and path_slots as for a render, segments = samples, shadow_rays = 0,
 * draws = 2 * samples, rejected = 0, schedule = XRT_SCHED_AOV, the launch under XRT_K_STEP.
 * A multi-device context shards rows as for a render and assembles every requested plane on
 * devices[0]. */
typedef struct { float* albedo; float* normal; float* depth; float* alpha; int32_t* object; } xrt_aov_buffers;
/* into caller-owned HOST memory; blocks until done */
int  xrt_render_aov(xrt_ctx* ctx, const xrt_render_params* p, const xrt_aov_buffers* host_out, xrt_stats* st);
/* into DEVICE pointers on this context's GPU (devices[0]); ordering as xrt_render_device_after:
 * waits only for the work queued so far on hip_stream (NULL = the legacy default stream) */
int  xrt_render_aov_device(xrt_ctx* ctx, const xrt_render_params* p, const xrt_aov_buffers* device_out,
                           void* hip_stream, xrt_stats* st);

/* ---- denoiser: edge-avoiding a-trous filter over a frame and its guide buffers -------- */
/* Dammertz et al. 2010: `iterations` passes of a 5 x 5 B3-spline kernel with tap spacing 1, 2, 4,
 * ... pixels; each tap is weighted by how far colour, shading normal, depth and albedo are from the
 * centre pixel's and cut to zero across an object-id boundary.  There is no albedo demodulation
 * (albedo is constant per object and the object stop already separates objects).
 * Inputs, in Image::pixels order: color [H][W][3] and the planes xrt_render_aov makes — albedo,
 * normal [H][W][3], depth [H][W], object [H][W] int32; alpha is ignored.  A NULL plane behaves
 * exactly as a plane of zeros (object: all 0), a NULL `guides` as all planes NULL.
 * The arithmetic is IEEE float32, one rounding per operation, no fused multiply-add:
 *   inv_x = sigma_x > 0 ? 1.0f / (sigma_x * sigma_x) : +0.0f      (x = color, normal, depth, albedo)
 *   iteration i = 0 .. iterations - 1, tap spacing s = 1 << i:
 *     kc = inv_color * (float)(1u << 2 i)            the colour stop tightens by 2 per iteration
 *     kz = inv_depth * (1.0f / (float)(1u << 2 i))   sigma_depth: the depth change tolerated per
 *                                                    step of tap spacing, in world units
 *     kn = inv_normal, ka = inv_albedo
 *     for pixel p, with c the iteration's input colour (the caller's, then the previous output):
 *       acc = (+0, +0, +0); ws = +0
 *       for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = p + s (dx, dy), q inside the image:
 *         d2c = (dc.x dc.x + dc.y dc.y) + dc.z dc.z,  dc = c[p] - c[q]   (d2n, d2a alike)
 *         d2z = dz dz,  dz = depth[p] - depth[q]
 *         e = ((d2c kc + d2n kn) + d2z kz) + d2a ka
 *         w = expf(-e) * (h[dy + 2] h[dx + 2]),  h = {1/16, 1/4, 3/8, 1/4, 1/16}, expf glibc's
 *         if object[p] != object[q]: w = +0
 *         acc.ch = acc.ch + c[q].ch w;  ws = ws + w
 *       out[p].ch = acc.ch / ws
 * The centre tap runs at its place in the loop (e = +0, w = 9/64), so ws > 0 for finite input.
 * Input must be finite; a non-finite value in a pixel's window leaves that pixel unspecified.
 * out == color is allowed; partial overlap is unspecified.
 * color NULL: the framebuffer of the context's last xrt_render, as xrt_tonemap reads it
 * (XRT_ERR_STATE when there is none of that size).  No scene or camera is needed.  A multi-device
 * context filters on devices[0], where frames and planes are assembled.  XRT_ERR_INVALID: NULL
 * ctx, params or out; width or height 0; iterations 0 or above XRT_DENOISE_MAX_ITERATIONS. */
#define XRT_DENOISE_MAX_ITERATIONS 6
#define XRT_DENOISE_TILED_ITERATIONS 2   /* the first n iterations (steps 1, 2) take the LDS-tiled kernel */
enum {
    XRT_DENOISE_TIMING = 1u,   /* time the launches with HIP events (xrt_denoise_stats.kernel_ms) */
    XRT_DENOISE_NO_TILE = 2u   /* every iteration through the direct kernel; same results          */
};
typedef struct {
    uint32_t width, height, iterations;
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo;   /* <= 0: the term is off */
    uint32_t flags;            /* XRT_DENOISE_*                                                     */
} xrt_denoise_params;
typedef struct {
    double wall_ms;            /* host wall clock of the call                                       */
    double kernel_ms;          /* HIP-event time over all launches (XRT_DENOISE_TIMING), else 0     */
    uint32_t launches;         /* the prepass and one per iteration                                 */
    uint32_t tiled_iterations, direct_iterations;   /* iterations per kernel                        */
    uint32_t reserved;
} xrt_denoise_stats;
/* caller-owned HOST memory; blocks until done */
int  xrt_denoise(xrt_ctx* ctx, const xrt_denoise_params* p, const float* color, const xrt_aov_buffers* guides,
                 float* out, xrt_denoise_stats* st);
/* DEVICE pointers on this context's GPU (devices[0]); ordering as xrt_render_aov_device: waits only
 * for the work queued so far on hip_stream (NULL = the legacy default stream) and returns when
 * d_out is complete */
int  xrt_denoise_device(xrt_ctx* ctx, const xrt_denoise_params* p, const float* d_color,
                        const xrt_aov_buffers* d_guides, float* d_out, void* hip_stream, xrt_denoise_stats* st);

/* ---- denoiser, variance-guided: the spatial filter of SVGF ---------------------------- */
/* Schied et al. 2017, section 4.3, without its temporal part: the a-trous filter above with the
 * absolute colour stop replaced by a luminance difference measured in standard deviations of the
 * centre pixel's own noise, and the variance filtered along with the colour, so every pass sees
 * how much noise the passes before it left.  The luminance factor is not tightened per pass (the
 * shrinking variance does that), so sigma_luminance is independent of the radiance scale and of
 * the iteration count.  color, the guide planes, out, their NULL rules, ordering on hip_stream,
 * the multi-device rule and xrt_denoise_stats are xrt_denoise's.  In addition
 *   variance     [H][W]  the variance of the pixel's luminance: finite and >= 0.  NULL: the
 *                        library estimates it from the frame (below)
 *   out_variance [H][W]  optional (NULL: not wanted): the variance left after the last pass
 * out == color and out_variance == variance are allowed; any other overlap is unspecified.
 * The arithmetic is IEEE float32, one rounding per operation, no fused multiply-add; expf is
 * glibc's, sqrtf and / are correctly rounded:
 *   lum(c) = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b
 *   the estimate (variance == NULL only), r = variance_radius, for pixel p:
 *     n = m1 = m2 = +0
 *     for dy = -r .. r (outer), dx = -r .. r (inner), q = p + (dx, dy), q inside the image and
 *     object[q] == object[p]:
 *       n = n + 1.0f;  m1 = m1 + lum(c[q]);  m2 = m2 + lum(c[q]) lum(c[q])
 *     mean = m1 / n;  v = m2 / n - mean mean;  var[p] = v > 0 ? v : +0
 *   (the centre tap always counts, so n >= 1: a spatial variance of the pixel's own object)
 *   inv_x = sigma_x > 0 ? 1.0f / (sigma_x * sigma_x) : +0.0f      (x = normal, depth, albedo)
 *   iteration i = 0 .. iterations - 1, tap spacing s = 1 << i:
 *     kz = inv_depth * (1.0f / (float)(1u << 2 i));  kn = inv_normal;  ka = inv_albedo
 *     for pixel p, with c and var the iteration's input (the caller's or the estimate, then the
 *     previous output):
 *       vs = gs = +0
 *       for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = p + (dx, dy), q inside the image:
 *         gw = g[dy + 1] g[dx + 1],  g = {1/4, 1/2, 1/4};  vs = vs + var[q] gw;  gs = gs + gw
 *       vg = vs / gs
 *       kl = sigma_luminance > 0 ? 1.0f / (sigma_luminance * sqrtf(vg) + 1e-8f) : +0.0f
 *       acc = (+0, +0, +0); vacc = +0; ws = +0
 *       for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = p + s (dx, dy), q inside the image:
 *         dl = fabsf(lum(c[p]) - lum(c[q]));  d2n, d2z, d2a as for xrt_denoise
 *         e = ((dl kl + d2n kn) + d2z kz) + d2a ka
 *         w = expf(-e) * (h[dy + 2] h[dx + 2]);  if object[p] != object[q]: w = +0
 *         acc.ch = acc.ch + c[q].ch w;  vacc = vacc + var[q] (w w);  ws = ws + w
 *       out[p].ch = acc.ch / ws;  var'[p] = vacc / (ws ws)
 * The centre tap gives ws >= 9/64 for finite input.  With sigma_luminance <= 0 the colour is
 * xrt_denoise's with sigma_color = 0, bit for bit.
 * XRT_ERR_INVALID and XRT_ERR_STATE as for xrt_denoise, and XRT_ERR_INVALID for a variance_radius
 * outside 1 .. XRT_DENOISE_VAR_MAX_RADIUS while variance is NULL.  xrt_denoise_stats.launches: the
 * prepass, the estimate when it ran, and one per iteration. */
#define XRT_DENOISE_VAR_MAX_RADIUS 3
#define XRT_DENOISE_VAR_TILED_ITERATIONS 2   /* the first n iterations (steps 1, 2) take the LDS-tiled kernel */
typedef struct {
    uint32_t width, height, iterations;        /* iterations: 1 .. XRT_DENOISE_MAX_ITERATIONS        */
    float sigma_luminance, sigma_normal, sigma_depth, sigma_albedo;   /* <= 0: the term is off */
    uint32_t variance_radius;  /* 1 .. 3: the estimate's window, read only when `variance` is NULL  */
    uint32_t flags;            /* XRT_DENOISE_TIMING, XRT_DENOISE_NO_TILE                           */
} xrt_denoise_var_params;
/* caller-owned HOST memory; blocks until done */
int  xrt_denoise_var(xrt_ctx* ctx, const xrt_denoise_var_params* p, const float* color, const float* variance,
                     const xrt_aov_buffers* guides, float* out, float* out_variance, xrt_denoise_stats* st);
/* DEVICE pointers on this context's GPU (devices[0]); ordering as xrt_denoise_device */
int  xrt_denoise_var_device(xrt_ctx* ctx, const xrt_denoise_var_params* p, const float* d_color,
                            const float* d_variance, const xrt_aov_buffers* d_guides, float* d_out,
                            float* d_out_variance, void* hip_stream, xrt_denoise_stats* st);

/* ---- ray queries: Scene::intersect / Scene::occluded (Src/scene.cpp:190-211) ---------- */
/* One IntersectInfo (Src/ray.h:23-39) as Scene::intersect leaves a fresh one. */
typedef struct {
    int32_t hit;             /* the query's return value                                   */
    int32_t object;          /* hitObject: index in iteration order (-1: none)             */
    int32_t primitive;       /* mesh hits: the object's triangle that set surfaceInfo, else -1 */
    float t;                 /* IntersectInfo::t  (kInfinity = FLT_MAX when nothing wrote it) */
    float t1;                /* IntersectInfo::t1 (medium boxes)                           */
    float position[3], ng[3], ns[3], dpdu[3], dpdv[3];   /* SurfaceInfo                  */
    float barycentric[2];    /* SurfaceInfo::barycentric (u, v) of that triangle           */
} xrt_hit;
enum { XRT_QUERY_INTERSECT = 0, XRT_QUERY_OCCLUDED = 1 };
/* n rays rays[i] = {ox, oy, oz, dx, dy, dz} against the uploaded scene, on the GPU with the
 * render's own trace kernels: XRT_QUERY_INTERSECT fills out[i] like Scene::intersect on a
 * fresh IntersectInfo; XRT_QUERY_OCCLUDED sets out[i].hit = Scene::occluded(ray, tmax[i])
 * (tmax NULL: FLT_MAX) and leaves the other fields zero.  Blocks until done.
 * Directions need not be unit vectors.  The answers are the reference's, bit for bit, for
 * finite rays whose origins lie within XRT_EXACT_DIAGONALS scene diagonals of the scene
 * (XRT_EXACT_DIAGONALS_TRI for a scene of triangle meshes only) and a scene as far from the
 * world origin at the most (see xrt_upload_scene); from further away a hit within float
 * error of an object's silhouette may be reported as a miss. */
int  xrt_query(xrt_ctx* ctx, uint32_t n, const float* rays, const float* tmax, int32_t mode, xrt_hit* out);

/* Output stage: Image::gammaCorrection(gamma) then writePPM's 8-bit quantisation
 * (Src/image.h:80-114) on the device, for n_pixels float3 pixels: d_rgb is a DEVICE
 * pointer on this context's GPU, or NULL for the framebuffer of the last xrt_render;
 * rgb8_out is caller-owned HOST memory of 3 * n_pixels bytes (the R G B values writePPM
 * prints, in pixel order). */
int  xrt_tonemap(xrt_ctx* ctx, const float* d_rgb, uint32_t n_pixels, float gamma, uint8_t* rgb8_out);

/* ---- host scene layer (C facade over the C++ Scene API; no GPU needed) ------------- */
typedef struct xrt_hscene xrt_hscene;
xrt_hscene* xrt_hscene_create(void);
void xrt_hscene_destroy(xrt_hscene* s);
const char* xrt_hscene_last_error(const xrt_hscene* s);
/* Scene::loadObj (Src/scene.cpp:46-154): OBJ/MTL with tinyobjloader-v2 semantics */
int xrt_hscene_load_obj(xrt_hscene* s, const char* path);
/* Scene::addObj(name, make_unique<Mesh>(prims, Lambert(albedo))); tri_n may be NULL
 * (face normals, as loadObj does when the OBJ has no vn) */
int xrt_hscene_add_mesh(xrt_hscene* s, const char* name, const float* tri_v, const float* tri_n,
                        uint32_t n_tris, const float albedo[3]);
/* SphereMesh(center, radius, nTheta, nPhi, Lambert(albedo)) (Src/primitive.cpp:170-205) */
int xrt_hscene_add_sphere_mesh(xrt_hscene* s, const char* name, const float center[3], float radius,
                               int n_theta, int n_phi, const float albedo[3]);
/* Sphere(center, radius, Lambert(albedo)) (Src/primitive.h:97-184) */
int xrt_hscene_add_sphere(xrt_hscene* s, const char* name, const float center[3], float radius,
                          const float albedo[3]);
/* Scene::addAreaLight(name, QuadLight/TriangleLight/SphereLight(..., Matrix44f(), Le)) */
int xrt_hscene_add_quad_light(xrt_hscene* s, const char* name, const float v0[3], const float v1[3],
                              const float v2[3], const float Le[3]);
int xrt_hscene_add_triangle_light(xrt_hscene* s, const char* name, const float v0[3],
                                  const float v1[3], const float v2[3], const float Le[3]);
int xrt_hscene_add_sphere_light(xrt_hscene* s, const char* name, const float center[3], float radius,
                                const float Le[3]);
/* the same SphereLight as the reference compiled with AREA_SAMPLING (XRT_LIGHT_SPHERE_AREA) */
int xrt_hscene_add_sphere_light_area(xrt_hscene* s, const char* name, const float center[3], float radius,
                                     const float Le[3]);
/* Scene::addObj(name, medium->makeObject()): a BoxMesh over the medium's bounds */
int xrt_hscene_add_medium_box(xrt_hscene* s, const char* name, const float pmin[3], const float pmax[3]);
/* Scene::addDeltaLight(name, PointLight / DistantLight(l2w, color, intensity)): l2w is the
 * row-major lightToWorld; pos / dir are computed as the reference constructors do */
int xrt_hscene_add_point_light(xrt_hscene* s, const char* name, const float l2w[16], const float color[3],
                               float intensity);
int xrt_hscene_add_distant_light(xrt_hscene* s, const char* name, const float l2w[16], const float color[3],
                                 float intensity);
/* Scene::getDeltaLights() flattened, in push-back order; valid until the next mutation */
int xrt_hscene_delta_lights(xrt_hscene* s, const xrt_delta_light** out, uint32_t* n);
/* Re-tag the object `object_name` (added earlier) with a material whose materialType() is the
 * one XRT_MAT_* names: Lambert keeps the object's albedo (0 if it had none), NONE drops it */
int xrt_hscene_set_material(xrt_hscene* s, const char* object_name, int32_t material);
/* Flatten in unordered_map iteration order.  Pointers stay valid until the next
 * mutation or destroy. */
int xrt_hscene_flatten(xrt_hscene* s, xrt_scene_desc* out);
/* Name of the i-th object in iteration order (NULL if out of range). */
const char* xrt_hscene_object_name(const xrt_hscene* s, uint32_t i);

/* PinholeCamera(aspect, c2w, FOV) -> scale = tan(0.5f*deg2rad(FOV)) (Src/camera.h:45) */
float xrt_pinhole_scale(float fov_deg);

/* ---- device self-tests (used by tests/, never by render) ------------------------- */
/* libstdc++ mt19937 + generate_canonical<float,24> draws for seeds[i], n draws each,
 * taken at stream offset `skip`: out[i*n + k] */
int xrt_test_rng(xrt_ctx* ctx, const uint32_t* seeds, uint32_t n_seeds, uint32_t skip, uint32_t n,
                 float* out);
/* glibc-sinf/cosf restatement on device over x[i]: out[2i] = sinf, out[2i+1] = cosf */
int xrt_test_trig(xrt_ctx* ctx, const float* x, uint32_t n, float* out);
/* exhaustive: count φ = 2π·r over every reachable draw value r where the device
 * restatement differs from the host values supplied by the caller in chunks. */
int xrt_test_trig_draw_domain(xrt_ctx* ctx, uint32_t first_bits, uint32_t count, float* out_sin,
                              float* out_cos, float* out_r);
/* glibc-logf/expf restatement on device over x[i]: out[2i] = logf, out[2i+1] = expf */
int xrt_test_logexp(xrt_ctx* ctx, const float* x, uint32_t n, float* out);
/* glibc-powf restatement on device: out[i] = powf(x[i], y) */
int xrt_test_powf(xrt_ctx* ctx, const float* x, uint32_t n, float y, float* out);
/* every 32-bit input: mode 0 checks the device's fast correctly rounded reciprocal against
 * 1.0f / b, mode 1 its division by the constant c (rc = 1.0f / c) against x / c; returns the
 * mismatch count and up to 16 mismatching inputs (0xffffffff = unused) */
int xrt_test_fastdiv(xrt_ctx* ctx, uint32_t mode, float c, float rc, uint64_t* n_bad, uint32_t* first_bad16);
/* k_whitted's own reflect / refract / fresnel / normalize (Src/geometry.cpp:13-16,52-89, ior
 * 1.3) over in[i] = {I.xyz, N.xyz}: out[i] = {reflect.xyz, refract.xyz, kr, normalize(reflect).xyz,
 * normalize(refract).xyz} (13 floats) */
int xrt_test_whitted_math(xrt_ctx* ctx, const float* in, uint32_t n, float* out);
/* The camera lists of the speculative merged schedule (k_camlist) for the uploaded scene and
 * camera and p's image and row shard, as a render of p would build them, without its retirement
 * of the empty pixels: out[4 s .. 4 s + 3] = {list bits 0-31, bits 32-63, the covering triangle
 * or 0xffffffff, 0} of slot s — column s % width, row shard_index + shard_count * (s / width);
 * the bits and the covering triangle count triangles in object order.  XRT_ERR_STATE unless the
 * scene is a triangle scene of 1 to 64 triangles.  Nothing a later render reads is left changed. */
int xrt_test_camlist(xrt_ctx* ctx, const xrt_render_params* p, uint32_t* out);
/* The slot -> pixel map (csrc/slot_map.h) a render of p would use, read back from the device
 * function the kernels call: out[s] = col + width * row of slot s, for the n slots of p's row
 * shard.  The row-major map gives out[s] = s for an unsharded image.  Needs an uploaded scene and
 * a camera (the schedule, and with it the map, depends on the scene); renders nothing.
 * xrt_test_camlist above is not affected by the map: its lists are always built under the
 * row-major one, slot s = pixel s, whatever p's flags say. */
int xrt_test_slot_map(xrt_ctx* ctx, const xrt_render_params* p, uint32_t* out);
/* The chunk phase the render of p would run (csrc/step_chunks.h), a device self-test: plan[0] = 1 if
 * it keeps its whole-wave phase in chunks, else 0 and nothing else is done; plan[1] = passes per block
 * per launch; then, after seeding and building the chunks as the render does, plan[2] = the chunks
 * that hold a slot, plan[3] = the blocks of a launch, and sizes[c] = live slots of chunk c for
 * c < min(n_sizes, plan[4]), plan[4] = the chunks the buffers hold (numbered 8 j + class). */
int xrt_test_chunk_plan(xrt_ctx* ctx, const xrt_render_params* p, uint32_t plan[5], uint32_t* sizes, uint32_t n_sizes);
/* How the volumetric kernels read the context's heterogeneous density grid: the per-cell corner
 * values (a dense grid whose cells take at most the corner limit, 2 GiB), four rows of the dense
 * grid itself (a larger one, or one without a cell), or leaf bricks (xrt_set_medium_bricks). */
enum { XRT_DENSITY_CORNERS = 0, XRT_DENSITY_ROWS = 1, XRT_DENSITY_BRICKS = 2 };
/* The kernels' own density lookup (HeterogeneousMedium::getDensity, multiplier included) of the
 * context's current medium at the world points points[3 i ..] = {x, y, z}, one lane per point:
 * out[i]; *layout = the XRT_DENSITY_* in use.  n = 0 only reports the layout.  XRT_ERR_STATE without
 * a medium or with a homogeneous one.  Exact where the points' index-space coordinates fit an int. */
int xrt_test_density(xrt_ctx* ctx, const float* points, uint32_t n, float* out, int32_t* layout);
/* The corner limit of later xrt_set_medium calls on this context (every device of a multi-device
 * one): a dense grid builds its corner values when (nx-1)(ny-1)(nz-1) * 32 <= max_bytes, so 0
 * makes every grid read its rows.  The results of a render never depend on it. */
int xrt_test_corner_grid_limit(xrt_ctx* ctx, uint64_t max_bytes);
/* The kernels' own HenyeyGreenstein::sampleDirection (Src/medium.h:37-67) over n items: wi[3 i ..]
 * for g and wo[3 i ..], and Medium::sampleWavelength (Src/medium.h:102-115): channel[i] and
 * pmf[3 i ..] for thr[3 i ..] and albedo[3 i ..].  Item i's stream is its own eight raw mt19937
 * state words words[8 i ..] (the generator's output is their tempering), read from the first. */
int xrt_test_hg(xrt_ctx* ctx, float g, const float* wo, const uint32_t* words, uint32_t n, float* wi);
int xrt_test_wavelength(xrt_ctx* ctx, const float* thr, const float* albedo, const uint32_t* words, uint32_t n,
                        uint32_t* channel, float* pmf);
/* What the last xrt_upload_scene built for the kernels that walk a hierarchy (csrc/bvh.h), read from
 * the context; nothing is launched.  out = {nodes of the triangle BVH, stack entries per ray of its
 * binary walk (tree depth + 1, at most 24), nodes of its 4-wide form, stack entries of that walk
 * (3 * depth + 1, at most 48; both 0 unless the scene is two-level), 1 if the scene is two-level,
 * nodes of the threaded sphere BVH, triangles in the triangle BVH (those with a zero edge vector are
 * left out), bytes per stack entry (2 or 4) of the walk the scene's deep rays take — the 4-wide one
 * of a two-level scene, else the binary one}; all 0 for a scene without the structure.
 * XRT_ERR_STATE without an uploaded scene. */
int xrt_test_bvh_info(xrt_ctx* ctx, int32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* XRT_H */
