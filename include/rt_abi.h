/*
 * rt_abi.h — C ABI of the MI355X path-tracing hot path.
 *
 * This is the drop-in boundary for juhotuho10/rust_GPU_raytracing's per-frame
 * compute path. In the reference, `Renderer` (src/renderer.rs) owns a
 * `DataBuffers` (src/buffers.rs) of 10 wgpu buffers + 2 textures and records
 * one compute pass of `compute_shader.wgsl::main` per frame. Here the same
 * surface is a handful of `extern "C"` functions over an opaque context that
 * owns hipMalloc'd buffers, a pinned staging ring and one HIP stream. The
 * Rust side would bind these with a plain `extern "C" { ... }` block (see
 * INTEGRATION.md); nothing in the signatures is a C++ or torch type.
 *
 * POD layouts below are byte-for-byte the reference's `#[repr(C)]` structs
 * (src/buffers.rs:7-129) — the host arrays the reference already builds can be
 * handed over with no conversion.
 *
 * Conventions
 *   - every call returns int: RT_OK (0) or a negative RT_E* code; the message
 *     of the last failure is available from rt_last_error(ctx).
 *   - host arrays passed in are copied before the call returns (async copies
 *     go through the context's pinned staging ring); the caller keeps
 *     ownership.
 *   - one context = one device + one stream; calls on one context are not
 *     thread-safe (the reference's Renderer is owned by the event-loop thread,
 *     src/main.rs:240-496).
 *   - all device work is stream-ordered, exactly like wgpu queue submission
 *     order (src/renderer.rs:249): an update issued before rt_compute_frame is
 *     visible to that frame's dispatch.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RT_API __attribute__((visibility("default")))
#else
#define RT_API
#endif

/* History: ... 11 (device display copy, default frame batch), 12 (tuning keys instead of
 * environment variables); 12, additive: ray queries (rt_trace_rays, rt_trace_rays_device,
 * rt_pick, rt_query_ray, rt_hit -- nothing earlier changed, so the number stays); 12,
 * additive: occlusion queries (rt_occluded, rt_occluded_device, rt_occlusion_ray); 12,
 * additive: denoiser (rt_compute_features, rt_read_features, rt_features_device, rt_denoise,
 * rt_read_denoised, rt_copy_denoised_to_device, rt_denoise_params);
 * 12, additive: radiance queries (rt_radiance, rt_radiance_device, rt_radiance_ray);
 * 12, additive: temporal denoiser (rt_denoise_temporal, rt_temporal_reset, rt_read_temporal,
 * rt_temporal_default_params, rt_temporal_params);
 * 12, additive: gather queries (rt_gather, rt_gather_device, rt_gather_point);
 * 12, additive: display transform (rt_display, rt_read_display, rt_copy_display_to_device,
 * rt_display_state, rt_display_reset, rt_display_default_params, rt_display_params);
 * 12, additive: probe queries (rt_probe_sh, rt_probe_sh_device, rt_probe);
 * 12, additive: ambient queries (rt_ambient, rt_ambient_device, rt_ambient_point);
 * 12, additive: motion records for the temporal denoiser (rt_denoise_temporal_motion, rt_motion,
 * rt_motion_from_transforms, rt_read_feature_ids, rt_feature_ids_device);
 * 12, additive: lens queries (rt_lens, rt_lens_device, rt_lens_rays, rt_lens_rays_device,
 * rt_lens_camera);
 * 12, additive: hit-list queries (rt_trace_hits, rt_trace_hits_device, rt_pick_hits,
 * RT_HITS_MAX);
 * 12, additive: proximity queries (rt_nearest, rt_nearest_device, rt_near_point,
 * struct rt_nearest). */
#define RT_ABI_VERSION 12

/* ---- error codes ------------------------------------------------------- */
#define RT_OK 0
#define RT_E_INVALID -1   /* bad argument (null, size mismatch, index out of range) */
#define RT_E_HIP -2       /* HIP runtime call failed */
#define RT_E_NOMEM -3     /* host or device allocation failed */
#define RT_E_CAPACITY -4  /* update larger than the buffer created at rt_create (wgpu would panic) */
#define RT_E_NODEVICE -5  /* no HIP device / device index out of range */

/* ---- POD scene types: src/buffers.rs:7-129 ----------------------------- */

/* src/buffers.rs:9-22 (Params) / compute_shader.wgsl:43-58. 48 bytes. */
typedef struct rt_params {
    uint32_t screen_width;
    uint32_t accumulation_index;
    uint32_t accumulate;
    uint32_t sphere_count;
    uint32_t object_count;
    uint32_t compute_per_frame;
    uint32_t texture_width;
    uint32_t texture_height;
    uint32_t texture_count; /* `textue_count` in the reference */
    uint32_t env_map_width;
    uint32_t env_map_height;
    uint32_t _padding;
} rt_params;

/* src/buffers.rs:26-29 (RayCamera). 16 bytes. */
typedef struct rt_ray_camera {
    float origin[3];
    uint32_t _padding;
} rt_ray_camera;

/* src/buffers.rs:33-36 (Ray): a cached per-pixel camera ray direction. 16 bytes. */
typedef struct rt_ray {
    float direction[3];
    uint32_t _padding;
} rt_ray;

/* src/buffers.rs:40-45 (SceneSphere). 32 bytes. */
typedef struct rt_scene_sphere {
    float position[3];
    float radius;
    uint32_t material_index;
    uint32_t _padding[3];
} rt_scene_sphere;

/* src/buffers.rs:49-64 (SceneTriangle), built by SceneTriangle::new
 * (src/buffers.rs:66-95): edge_ab = b-a, edge_ac = c-a,
 * calc_normal = edge_ab x edge_ac, face_normal = normalize(calc_normal).
 * 112 bytes. min/max_bounds are host-only (the kernel never reads them). */
typedef struct rt_scene_triangle {
    float a[3];           uint32_t _padding0;
    float edge_ab[3];     uint32_t _padding1;
    float edge_ac[3];     uint32_t _padding2;
    float calc_normal[3]; uint32_t _padding3;
    float face_normal[3]; uint32_t _padding4;
    float min_bounds[3];  uint32_t _padding5;
    float max_bounds[3];  uint32_t _padding6;
} rt_scene_triangle;

/* src/buffers.rs:100-109 (SceneMaterial). 32 bytes. */
typedef struct rt_scene_material {
    uint32_t texture_index;
    float roughness;
    float emission_power;
    float specular;
    float specular_scatter;
    float glass;
    float refraction_index;
    uint32_t _padding;
} rt_scene_material;

/* src/buffers.rs:113-120 (ObjectInfo). 48 bytes. */
typedef struct rt_object_info {
    float min_bounds[3];
    uint32_t first_sub_object_index;
    float max_bounds[3];
    uint32_t sub_object_count;
    uint32_t material_index;
    uint32_t _padding[3];
} rt_object_info;

/* src/buffers.rs:124-129 (SubObjectInfo). 32 bytes. */
typedef struct rt_sub_object_info {
    float min_bounds[3];
    uint32_t first_triangle_index;
    float max_bounds[3];
    uint32_t triangle_count;
} rt_sub_object_info;

/* ---- context ------------------------------------------------------------ */

typedef struct rt_ctx rt_ctx;

/* Everything DataBuffers::new (src/buffers.rs:159-170) receives, plus the
 * framebuffer height (Params carries only the width) and the device.
 * Array capacities are fixed here, as wgpu buffer sizes are fixed at
 * creation; later rt_update_* calls must fit. Zero-length arrays are allowed
 * (the reference needs a dummy element because WGSL arrays cannot be empty). */
typedef struct rt_create_info {
    uint32_t width;
    uint32_t height;
    int32_t device;              /* HIP device ordinal */
    uint32_t _reserved;
    rt_ray_camera camera;        /* binding 3 */
    const rt_ray* camera_rays;   /* binding 1, width*height entries */
    const rt_scene_material* materials; uint32_t material_count;   /* binding 4 */
    const rt_scene_sphere* spheres;     uint32_t sphere_count;     /* binding 5 */
    const rt_scene_triangle* triangles; uint32_t triangle_count;   /* binding 7 */
    const rt_object_info* objects;      uint32_t object_count;     /* binding 8 */
    const rt_sub_object_info* sub_objects; uint32_t sub_object_count; /* binding 10 */
    rt_params params;            /* binding 0: initial Params (Renderer::new, src/main.rs:131-144) */
    /* Tile partition for multi-GPU: the image is cut into 8x8
     * pixel tiles, tile t is rendered by rank (t % world_size). A context
     * with world_size == 1 renders every pixel, as the reference does. */
    uint32_t rank;
    uint32_t world_size;
} rt_create_info;

/* Renderer::new -> DataBuffers::new (src/renderer.rs:42-101,
 * src/buffers.rs:159-298). Allocates and fills every device buffer. Unlike the
 * reference (accumulation created uninitialised, src/buffers.rs:217-222) the
 * accumulation buffer starts zeroed. The renderer's accumulation counter k
 * starts at 1 (src/renderer.rs:96). */
RT_API int rt_create(const rt_create_info* info, rt_ctx** out_ctx);
RT_API void rt_destroy(rt_ctx* ctx);
RT_API const char* rt_last_error(const rt_ctx* ctx); /* never NULL; "" when no error */
RT_API int rt_abi_version(void);
/* Identity of this build: the hash of the sources, headers and compiler flags it
 * was compiled from (rust_gpu_raytracing_amd/build.py: source_hash). */
RT_API const char* rt_build_hash(void);

/* DataBuffers::update_texture_buffer (src/buffers.rs:479-511): `layers`
 * RGBA8 (sRGB-encoded, Rgba8UnormSrgb) images of width x height, tightly
 * packed, row 0 first. Resizes the texture array when the size changes. */
RT_API int rt_upload_textures(rt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t layers);
/* DataBuffers::update_environment_map_buffer (src/buffers.rs:513-539). */
RT_API int rt_upload_env_map(rt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height);

/* DataBuffers::update_accumulation (src/buffers.rs:557-559): write Params. */
RT_API int rt_update_params(rt_ctx* ctx, const rt_params* params);
/* DataBuffers::reset_accumulation (src/buffers.rs:545-555): zero the
 * accumulation buffer and write Params; also resets the context's
 * accumulation counter to params->accumulation_index (Renderer sets it to 1,
 * src/renderer.rs:131-151). */
RT_API int rt_reset_accumulation(rt_ctx* ctx, const rt_params* params);

/* DataBuffers::update_* (src/buffers.rs:541-595) and the camera write in
 * Renderer::on_update (src/renderer.rs:116-125). Writes start at element 0;
 * `count` must not exceed the capacity given at rt_create. */
RT_API int rt_update_ray_directions(rt_ctx* ctx, const rt_ray* rays, uint32_t count);
RT_API int rt_update_camera(rt_ctx* ctx, const rt_ray_camera* camera);

/* Device-side primary rays: instead of reading camera_rays,
 * the kernel computes each pixel's direction with the per-pixel arithmetic of
 * Camera::recalculate_ray_directions (src/camera.rs:139-182) from the camera's
 * inverse projection and inverse view (column-major 4x4 f32, glam layout), in
 * f32 with glam's operation order -- the same bits the host generator would
 * upload. Stays in effect until the next rt_update_ray_directions. */
RT_API int rt_update_camera_matrices(rt_ctx* ctx, const float inverse_projection[16], const float inverse_view[16]);
RT_API int rt_update_spheres(rt_ctx* ctx, const rt_scene_sphere* spheres, uint32_t count);
RT_API int rt_update_triangles(rt_ctx* ctx, const rt_scene_triangle* triangles, uint32_t count);
RT_API int rt_update_object_info(rt_ctx* ctx, const rt_object_info* objects, uint32_t count);
RT_API int rt_update_sub_object_info(rt_ctx* ctx, const rt_sub_object_info* sub_objects, uint32_t count);
RT_API int rt_update_materials(rt_ctx* ctx, const rt_scene_material* materials, uint32_t count);

/* The compute pass of Renderer::compute_frame (src/renderer.rs:238-249):
 * one launch of the path-tracing kernel with the Params currently on the
 * device. `bounces` is the per-path bounce limit (the reference hard-codes
 * 10, compute_shader.wgsl:150). Asynchronous. */
RT_API int rt_dispatch(rt_ctx* ctx, uint32_t bounces);

/* Renderer::compute_frame (src/renderer.rs:201-252): if Params.accumulate
 * is 1, write Params with accumulation_index = k and then k += 1; then
 * rt_dispatch. Asynchronous. With frame batching (below) the frame may only be
 * queued: an error of its launch (a failed allocation or launch) is then returned
 * by the call that launches the batch -- the rt_compute_frame that fills it, or
 * the next other entry point on the context. */
RT_API int rt_compute_frame(rt_ctx* ctx, uint32_t bounces);

/* `frames` consecutive rt_compute_frame calls fused into one launch: each
 * pixel runs its frames back to back on one lane, so the accumulation, the
 * packed output and the ray count afterwards are exactly those of the
 * sequence of calls (the per-frame outputs in between are never observable:
 * the reference only reads output_data after a frame, src/renderer.rs:254).
 * Used by the multi-GPU bench, where each rank advances its tiles by N frames
 * per step. frames >= 1. A batch whose per-frame buffers (32 B per owned pixel,
 * frame and sample) would exceed the batch budget -- an eighth of the device's
 * memory, tuning "batch_memory_mb" -- runs as consecutive launches of as many
 * frames as fit, with the same results. Asynchronous. */
RT_API int rt_compute_frames(rt_ctx* ctx, uint32_t bounces, uint32_t frames);

/* `count` consecutive rt_compute_frame calls made in one call (new, ABI 10): the loop a
 * native host runs around rt_compute_frame, for callers whose per-call overhead is not
 * negligible (the Python mirror: ~2 us per ctypes call, 40 us per 20-frame bench step at
 * N GPUs, where a rank's launch is 0.7 ms). Frame batching applies exactly as to the single
 * calls; results are identical. Stops at the first failing call. Asynchronous. */
RT_API int rt_submit_frames(rt_ctx* ctx, uint32_t bounces, uint32_t count);

/* Frame batching (new; the reference submits one dispatch per compute_frame,
 * src/renderer.rs:238-249, and wgpu runs it later, asynchronously). With
 * max_frames > 1, rt_compute_frame queues its frame (Params and k advance as
 * always) and one launch renders the queued frames once max_frames are queued,
 * when the bounce count changes, or before ANY other call on the context
 * (readback, update, sync, timing, destroy). Every frame is traced in full.
 * Accumulating batches are frame-parallel: each (frame, 8x8 tile) is a unit of
 * the launch's work queue, each path's light goes to a per-(frame, sample)
 * buffer, and a resolve pass adds them to the accumulation in the reference's
 * order (frame k's samples, then frame k+1's: compute_shader.wgsl:156-164), so
 * the accumulation, the packed output, the ray count and k after the batch are
 * bit-identical to the single-frame dispatches'; what changes is that the
 * persistent grid's fill and drain are paid once per batch, and that a tile
 * split over N GPUs keeps N x the units per launch. Non-accumulating batches
 * (every frame the same frame) run each pixel's frames back to back on a lane.
 * The default is RT_DEFAULT_FRAME_BATCH (ABI 11; it was 1, one launch per frame): a
 * host that mirrors the reference's event loop -- one rt_compute_frame per frame and
 * a display copy every few frames (src/renderer.rs:201-283, src/main.rs:88-92,
 * 365-375) -- gets launches of the frames between two displays without calling
 * this. 1 launches each frame at once.
 * max_frames in [1, 64]. rt_frame_batch reports the setting and the frames
 * queued; rt_flush launches them now. */
#define RT_DEFAULT_FRAME_BATCH 16
RT_API int rt_set_frame_batch(rt_ctx* ctx, uint32_t max_frames);
RT_API int rt_frame_batch(const rt_ctx* ctx, uint32_t* max_frames, uint32_t* pending);
RT_API int rt_flush(rt_ctx* ctx);

/* Blocks until all work on the context's stream has finished. */
RT_API int rt_synchronize(rt_ctx* ctx);

/* ---- ray queries (ABI 12, additive: ray queries) ---------------------------
 *
 * "What does this ray hit?" for arbitrary rays, answered by the closest-hit search the
 * path tracer runs for every path segment (the exact-culling sphere BVH, the certified
 * triangle accelerator, the brute-force set): trace_ray of the reference
 * (compute_shader.wgsl:342-353) as a batched call. Every record is bit-identical to the
 * reference's sweep over all primitives.
 *
 * Both records are laid out for 16-byte vector loads and stores. */

/* One ray. Directions need not be unit length; the pads are ignored. 32 bytes. */
typedef struct rt_query_ray {
    float origin[3];
    float _pad0;
    float direction[3];
    float _pad1;
} rt_query_ray;

/* The closest hit of one ray (HitPayload, compute_shader.wgsl:128-137, plus what was hit).
 * A miss is all-zero apart from t. 64 bytes. */
#define RT_HIT_MISS 0u
#define RT_HIT_SPHERE 1u
#define RT_HIT_TRIANGLE 2u
typedef struct rt_hit {
    float t;                 /* hit distance in units of |direction|; 3.4028235e38f on a miss */
    float position[3];       /* origin + direction * t */
    float normal[3];         /* unit, facing the ray */
    float u;                 /* texture coordinates (sphere_texture_coords / object_texture_coords) */
    float v;
    uint32_t material_index;
    uint32_t front_face;     /* 0 or 1 */
    uint32_t kind;           /* RT_HIT_MISS, RT_HIT_SPHERE, RT_HIT_TRIANGLE */
    uint32_t index;          /* sphere index as uploaded with rt_update_spheres, or object index */
    uint32_t sub_object;     /* triangle hits: index into the sub-object buffer; else 0 */
    uint32_t triangle;       /* triangle hits: index into the triangle buffer; else 0 */
    uint32_t _reserved;      /* 0 */
} rt_hit;

#if defined(__cplusplus)
static_assert(sizeof(rt_query_ray) == 32, "rt_query_ray is 32 bytes");
static_assert(sizeof(rt_hit) == 64, "rt_hit is 64 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_query_ray) == 32, "rt_query_ray is 32 bytes");
_Static_assert(sizeof(rt_hit) == 64, "rt_hit is 64 bytes");
#endif

/* Traces `count` rays and writes one record per ray, in order.
 *
 * A query sees the scene as of the call: after every earlier rt_update_*,
 * rt_set_object_models and rt_update_objects, with the accelerators prepared exactly as a
 * dispatch prepares them. It changes nothing a render can observe: not the accumulation,
 * the output, the accumulation index, the frames queued by rt_compute_frame (they stay
 * queued: rt_frame_batch reports the same `pending`), rt_ray_count, the timing totals or
 * the tile schedule. Results do not depend on the brute-force mode, on any rt_set_tuning
 * key or on triangle pruning modes 0 and 1 (mode 2 is inexact for queries as for frames).
 *
 * Exactness holds for the domain the culling bounds are derived for (DESIGN.md §5.2,
 * §5.3c): finite components, |direction| in [1e-5, 1e5], |origin| <= 1e15. Outside it the
 * record is unspecified; the search still terminates (the walks' skip links only advance).
 * What makes tiny directions inexact is the slab test's reciprocal cap: |1/d| is held at 1e30
 * per axis, and once it binds on more than one axis the box distances no longer follow the
 * ray, so normalise a direction of unknown length rather than rely on the margin below 1e-5.
 *
 * rt_trace_rays: host pointers, synchronous. Rays and records are staged through pinned
 * memory in chunks of tuning "query_chunk" rays, so `count` is not limited by a scratch
 * allocation.
 * rt_trace_rays_device: device pointers on the context's device, 16-byte aligned;
 * stream-ordered on rt_stream(ctx), no host copy, asynchronous. RT_E_INVALID when either
 * is not device memory of the context's device.
 * count == 0 returns RT_OK and launches nothing; NULL pointers with count > 0 are
 * RT_E_INVALID. */
RT_API int rt_trace_rays(rt_ctx* ctx, const rt_query_ray* rays, rt_hit* hits, uint64_t count);
RT_API int rt_trace_rays_device(rt_ctx* ctx, const void* rays_device, void* hits_device, uint64_t count);

/* The closest hit of pixel (x, y)'s un-jittered camera ray: the camera origin plus that
 * pixel's direction, from the ray buffer (rt_update_ray_directions) or computed from the
 * camera matrices while rt_update_camera_matrices is in effect. RT_E_INVALID when x or y
 * is outside the framebuffer. Synchronous. */
RT_API int rt_pick(rt_ctx* ctx, uint32_t x, uint32_t y, rt_hit* hit);

/* ---- occlusion queries (ABI 12, additive: occlusion queries) ---------------
 *
 * "Is anything in the way before t_max?" for arbitrary rays: shadow rays, line of sight,
 * occlusion baking. An any-hit search: it stops at the first primitive that decides the
 * answer and culls by t_max from the first node, which a closest-hit query cannot. */

/* One ray with a distance bound. The layout of rt_query_ray with t_max in the place of
 * _pad1, so one buffer can be handed to rt_trace_rays (which ignores the pad) and to
 * rt_occluded. 32 bytes. */
typedef struct rt_occlusion_ray {
    float origin[3];
    float _pad0;        /* ignored */
    float direction[3]; /* need not be unit length */
    float t_max;        /* in units of |direction|, like rt_hit.t */
} rt_occlusion_ray;

#if defined(__cplusplus)
static_assert(sizeof(rt_occlusion_ray) == 32, "rt_occlusion_ray is 32 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_occlusion_ray) == 32, "rt_occlusion_ray is 32 bytes");
#endif

/* Writes one byte per ray, in order, exactly 0 or 1; no byte outside [0, count) is written.
 *
 * A ray is occluded (1) if and only if at least one primitive, tested on its own by the
 * reference's test, is accepted at a distance t with t < t_max in f32: the sphere test of
 * check_spheres (compute_shader.wgsl:355-404: disc >= 0, t > 0) or the triangle test of
 * check_triangles (:422-517, behind its object and sub-object ray_in_bounds: dist >= 0,
 * u, v, w >= 0). The answer does not depend on the order primitives are visited in and
 * no NaN takes part in it. Consequences:
 *  - For every ray whose closest-hit search meets no NaN distance, the byte equals
 *    `hit.kind != RT_HIT_MISS && hit.t < t_max` on the record rt_trace_rays returns for
 *    that ray. The comparison is strict: t_max == hit.t is NOT occluded.
 *  - t_max = +inf or 3.4028235e38f asks "is there any hit at all" (a hit as rt_trace_rays
 *    defines one: t < 3.4028235e38f). A miss is not occluded for any t_max.
 *  - t_max <= 0 or NaN gives 0.
 *  - A candidate whose distance is NaN never occludes: the measure-zero case of a ray lying
 *    exactly in a triangle's plane, which the reference's sweep accepts (:457). This is the
 *    one difference from the closest-hit record, whose t can be NaN there and then hides a
 *    sphere that does block the ray.
 *  - Exactness holds for the domain of the ray queries above: finite components,
 *    |direction| in [1e-5, 1e5], |origin| <= 1e15. Outside it the byte is unspecified; the
 *    search still terminates.
 *
 * Scene visibility and side effects are those of rt_trace_rays: the query sees the scene as
 * of the call, with the accelerators prepared exactly as a dispatch prepares them, and
 * changes nothing a render can observe (queued frames stay queued; the accumulation index,
 * rt_ray_count, the timing totals and the tile schedule are untouched). The bytes do not
 * depend on the brute-force mode, on any rt_set_tuning key or on triangle pruning modes 0
 * and 1 (mode 2 is inexact here as for frames and ray queries).
 *
 * rt_occluded: host pointers, synchronous. Staged through the pinned buffer of
 * rt_trace_rays in chunks of tuning "query_chunk" rays (32 bytes in, 1 byte out per ray).
 * rt_occluded_device: device pointers on the context's device; the rays 16-byte aligned,
 * the result at any alignment; stream-ordered on rt_stream(ctx), no host copy,
 * asynchronous. RT_E_INVALID when either is not device memory of the context's device.
 * Tuning "query_lds_mode" selects the scene placement as for the ray queries.
 * count == 0 returns RT_OK and launches nothing; NULL pointers with count > 0 are
 * RT_E_INVALID. */
RT_API int rt_occluded(rt_ctx* ctx, const rt_occlusion_ray* rays, uint8_t* occluded, uint64_t count);
RT_API int rt_occluded_device(rt_ctx* ctx, const void* rays_device, void* occluded_device, uint64_t count);

/* ---- hit-list queries (ABI 12, additive: hit-list queries) -----------------
 *
 * "What are the things along this ray, in order?" for arbitrary rays: the max_hits nearest
 * primitives of each ray, each as the rt_hit record of a closest-hit query. Click-through
 * picking, shadow rays attenuated by the glass they cross, thickness and crossing counts,
 * "is the camera inside an object". The input record is rt_occlusion_ray, so one buffer serves
 * rt_trace_rays, rt_occluded and rt_trace_hits; ray i's entries are
 * hits[i * max_hits .. i * max_hits + max_hits).
 *
 * THE HIT-LIST CONTRACT. For the ray (o, d, t_max) and a list length max_hits in 1..RT_HITS_MAX:
 *  1. Bound. bound = min(t_max, 3.4028235e38f). A t_max that is <= 0 or NaN gives no candidates.
 *  2. Sphere candidates. Sphere i is a candidate when the test of check_spheres
 *     (compute_shader.wgsl:355-404) on it alone accepts it: not disc < 0, and
 *     t = (-b - sqrt(disc)) / (2a) with t > 0; and t < bound. One candidate per sphere, the near
 *     root, as in the reference.
 *  3. Triangle candidates. A visit (object oi, sub-object slot i, triangle slot j) of the sweep of
 *     check_triangles (:422-517) is a candidate when it is behind the ray_in_bounds tests of its
 *     object and of its sub-object, with the reference's index clamps; none of the reference's
 *     rejections dist < 0, v < 0, u < 0, w < 0 holds (dist >= 0 and u, v, w >= 0); and its
 *     distance is not NaN and is < bound. Its sweep position seq is its position in the sweep's
 *     order over all (object, sub-object slot, triangle slot) triples, boxes disregarded.
 *  4. NaN distances. A candidate with a NaN distance is never listed: the any-hit rule, and the
 *     one difference from the closest-hit record.
 *  5. Order. Ascending t. At equal t triangles come before spheres, triangles ascend by seq and
 *     spheres ascend by index as uploaded: the order in which trace_ray (:342-353) and the two
 *     sweeps would prefer them.
 *  6. Result. n = min(number of candidates, max_hits). Entries 0..n-1 are the first n candidates
 *     in that order, each the rt_hit record rt_trace_rays builds for that primitive at that t:
 *     position, facing normal, u and v whatever the texture size, material, front_face, kind,
 *     index, sub_object, triangle. Entries n..max_hits-1 are the miss record: all zero,
 *     t = 3.4028235e38f. counts[i] = n. Every entry of every ray is written and nothing else is.
 *
 * Consequences:
 *  1. With t_max = +inf, entry 0 is the record of rt_trace_rays bit for bit, for every ray whose
 *     closest-hit search meets no NaN distance.
 *  2. counts[i] > 0 exactly when rt_occluded answers 1 for the same record, for any t_max.
 *  3. Lists nest: the list for max_hits = K is the first K entries of the list for any K' > K.
 *  4. counts saturates at max_hits. A caller that must know whether a list is complete asks for
 *     one entry more than it uses.
 *  5. The exactness domain, scene visibility and side effects are those of rt_trace_rays. There
 *     are no side effects: queued frames stay queued, and nothing a render observes changes. The
 *     result does not depend on the brute-force mode, on any rt_set_tuning key ("query_lds_mode"
 *     included) or on triangle pruning modes 0 and 1. It works on rank contexts. The search
 *     terminates on any input: the walks' skip links only advance.
 *
 * rt_trace_hits: host pointers, synchronous; `counts` may be NULL. Staged through the pinned
 * buffer of rt_trace_rays in chunks of max(1, "query_chunk" / max_hits) rays.
 * rt_trace_hits_device: device pointers on the context's device, rays and hits 16-byte aligned,
 * counts (may be NULL) 4-byte aligned; stream-ordered on rt_stream(ctx), no host copy,
 * asynchronous. While the call runs, the hits buffer also holds the lists being built.
 * rt_pick_hits: the list of pixel (x, y)'s un-jittered camera ray as rt_pick defines it, with
 * t_max = +inf; *n receives the count. Synchronous.
 * RT_E_INVALID: max_hits == 0 or > RT_HITS_MAX, whatever count is; NULL rays or hits with
 * count > 0 (rt_pick_hits: NULL hits or n); pointers that are not device memory of the context's
 * device, or misaligned (the device form); x or y outside the framebuffer. count == 0 returns
 * RT_OK and launches nothing. */
#define RT_HITS_MAX 16u
RT_API int rt_trace_hits(rt_ctx* ctx, const rt_occlusion_ray* rays, rt_hit* hits /* count * max_hits */,
                         uint32_t* counts /* count; may be NULL */, uint64_t count, uint32_t max_hits);
RT_API int rt_trace_hits_device(rt_ctx* ctx, const void* rays_device, void* hits_device,
                                void* counts_device /* may be NULL */, uint64_t count, uint32_t max_hits);
RT_API int rt_pick_hits(rt_ctx* ctx, uint32_t x, uint32_t y, rt_hit* hits /* max_hits */, uint32_t* n,
                        uint32_t max_hits);

/* ---- proximity queries (ABI 12, additive: proximity queries) ---------------
 *
 * "What is the closest surface point to this point?": snapping, clearance before a move, camera
 * collision, distance-field bakes, picking near a 3D cursor. Every other query starts from a ray;
 * this one starts from a point, against the same scene on the device.
 *
 * THE NEAREST-POINT CONTRACT. The reference has no such function, so the contract is this
 * library's. Every operation below is one f32 operation, rounded to nearest; nothing is
 * contracted into a fused multiply-add; division and sqrt are correctly rounded;
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z. For the point p and the bound max_distance:
 *
 *  1. Sphere i, centre c and radius r as uploaded (only |r| matters: hollow shells with a
 *     negative radius are spheres of radius |r|):
 *       v = c - p;  l = sqrt(dot(v, v));  key = | l - |r| |.
 *     If l == 0: point = (c.x + |r|, c.y, c.z), normal = (1, 0, 0). Otherwise s = |r| / l,
 *     point = c - v*s (per component c.k - v.k*s), normal = -(v / l) (per component -(v.k / l)).
 *     side = l >= |r| (1: on or outside the surface). feature = 0.
 *  2. Triangle, from the stored a, edge_ab (ab), edge_ac (ac); no vertex is rebuilt except as
 *     written. Ericson's seven regions in this order, with the textbook's <= and >=; a comparison
 *     with NaN is false, so the search falls through to the next region:
 *       ap = p - a;  d1 = dot(ab, ap);  d2 = dot(ac, ap)
 *       1 (vertex a):  d1 <= 0 && d2 <= 0:               q = a
 *       bp = ap - ab;  d3 = dot(ab, bp);  d4 = dot(ac, bp)
 *       2 (vertex b):  d3 >= 0 && d4 <= d3:              q = a + ab
 *       vc = d1*d4 - d3*d2
 *       3 (edge ab):   vc <= 0 && d1 >= 0 && d3 <= 0:    v = W(d1 / (d1 - d3));  q = a + ab*v
 *       cp = ap - ac;  d5 = dot(ab, cp);  d6 = dot(ac, cp)
 *       4 (vertex c):  d6 >= 0 && d5 <= d6:              q = a + ac
 *       vb = d5*d2 - d1*d6
 *       5 (edge ac):   vb <= 0 && d2 >= 0 && d6 <= 0:    w = W(d2 / (d2 - d6));  q = a + ac*w
 *       va = d3*d6 - d5*d4;  e1 = d4 - d3;  e2 = d5 - d6
 *       6 (edge bc):   va <= 0 && e1 >= 0 && e2 >= 0:    w = W(e1 / (e1 + e2));
 *                                                        q = (a + ab*(1 - w)) + ac*w
 *       7 (face):      denom = 1 / ((va + vb) + vc);  v = W(vb*denom);  w = W(vc*denom);
 *                      if (w > 1 - v) w = 1 - v;         q = (a + ab*v) + ac*w
 *     W(x) = x if 0 <= x <= 1, 1 if x > 1, else 0 (NaN included): every weight is in [0, 1], so
 *     q is a convex combination of the vertices whatever a degenerate triangle makes of the
 *     quotients -- that is what lets a box bound the key. A vector times a weight is one product
 *     per component; sums are taken left to right as parenthesised.
 *       key = sqrt(dot(q - p, q - p));  point = q;  normal = the stored face_normal, not flipped;
 *       side = dot(calc_normal, ap) >= 0;  feature = the region number, 1..7.
 *  3. Candidates: every sphere 0..sphere_count-1, and every triangle visit of the reference's
 *     sweep through objects 0..object_count-1 and their sub-objects, at its sweep position as THE
 *     HIT-LIST CONTRACT defines it (index clamps included). Object and sub-object boxes are not
 *     part of the meaning. A primitive is a candidate iff its key is not NaN and
 *     key <= max_distance: max_distance = +inf means "anything", a NaN or negative max_distance
 *     gives a miss, and so do NaN coordinates.
 *  4. Result: the candidate of the smallest key; among equal keys a triangle before a sphere (as
 *     trace_ray prefers them), then the lower sweep position or the lower sphere index.
 *     distance = its key. A miss is all zero apart from distance = 3.4028235e38f, as in rt_hit.
 *  5. Domain for exactness: finite position with |position| <= 1e15, as for ray origins. Outside
 *     it the record is unspecified; the search terminates on any input.
 *  6. The call sees the scene as of the call and changes nothing that a render, a queued frame,
 *     rt_ray_count, the timings or the tile schedule can observe. The result does not depend on
 *     the brute-force mode, on any rt_set_tuning key ("query_lds_mode" and "nearest_walk"
 *     included) or on the triangle pruning mode. It works on rank contexts.
 *
 * The accelerated search culls by the boxes of the sphere BVH and of the triangle accelerator
 * with a certified lower bound. Sub-object boxes come from the caller
 * (rt_update_sub_object_info) and carry no meaning here: while they are not known to enclose
 * their triangles and every triangle in a finite box to be finite -- the library looks once after
 * a triangle, sub-object or object-range upload and after rt_update_objects -- and in brute-force
 * mode, every candidate is tested instead. The result is the same. That look is a host pass: the
 * first rt_nearest or rt_nearest_device call after such an upload or edit, on a scene with
 * objects, copies every triangle back to the host and waits for the stream before it launches;
 * the calls after it do not.
 *
 * rt_nearest: host pointers, synchronous; staged through the pinned buffer of rt_trace_rays in
 * chunks of "query_chunk" points. rt_nearest_device: device pointers on the context's device,
 * 16-byte aligned; stream-ordered on rt_stream(ctx), no host copy of the records, asynchronous
 * but for the look at the boxes described above.
 * RT_E_INVALID: NULL points or out with count > 0; pointers that are not device memory of the
 * context's device, or misaligned (the device form). count == 0 returns RT_OK and launches
 * nothing. */
typedef struct rt_near_point {
    float position[3];
    float max_distance;      /* candidates have key <= max_distance; +inf: anything */
} rt_near_point;

/* (a tag only: the entry point carries the same name) */
struct rt_nearest {
    float distance;          /* the key; 3.4028235e38f on a miss */
    float point[3];          /* the closest surface point */
    float normal[3];         /* sphere: outward; triangle: the stored face_normal */
    uint32_t feature;        /* sphere: 0; triangle: the region, 1..7 */
    uint32_t kind;           /* RT_HIT_MISS, RT_HIT_SPHERE, RT_HIT_TRIANGLE */
    uint32_t index;          /* sphere index as uploaded, or object index */
    uint32_t sub_object;
    uint32_t triangle;
    uint32_t material_index;
    uint32_t side;           /* sphere: 1 on or outside; triangle: 1 on calc_normal's side */
    uint32_t _reserved[2];   /* 0 */
};
RT_API int rt_nearest(rt_ctx* ctx, const rt_near_point* points, struct rt_nearest* out, uint64_t count);
RT_API int rt_nearest_device(rt_ctx* ctx, const void* points_device, void* out_device, uint64_t count);

/* ---- radiance queries (ABI 12, additive: radiance queries) -----------------
 *
 * "How much light arrives along this ray?" for arbitrary rays: the path tracer's shading, RNG
 * and bounce loop (per_pixel, compute_shader.wgsl:210-314) started from a record instead of
 * the pinhole and a pixel. Irradiance and reflection probes, lightmap texels, thin-lens,
 * orthographic or panoramic cameras (a different origin per ray), the light at a picked point. */

/* One ray with its RNG stream. The layout of rt_query_ray with the RNG stream in the place of
 * _pad0: one buffer can be handed to rt_trace_rays, rt_occluded and rt_radiance. 32 bytes. */
typedef struct rt_radiance_ray {
    float origin[3];
    uint32_t stream;     /* takes the place of the pixel index in per_pixel's seed */
    float direction[3];  /* need not be unit length */
    float _pad1;         /* ignored */
} rt_radiance_ray;

#if defined(__cplusplus)
static_assert(sizeof(rt_radiance_ray) == 32, "rt_radiance_ray is 32 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_radiance_ray) == 32, "rt_radiance_ray is 32 bytes");
#endif

/* Writes four floats per ray, in order; nothing outside [0, 4 * count) is written.
 *
 * For ray i with record (o, stream, d):
 *
 *   R = (0.0f, 0.0f, 0.0f, 0.0f)
 *   for s = 0 .. samples-1, ascending:
 *       L = per_pixel(compute_shader.wgsl:210-314) with
 *             the camera origin replaced by o,
 *             camera_rays[index] replaced by d,
 *             seed = stream * (first_sample + s) * 326624u   (u32, wrapping; :217 with index := stream)
 *             the loop limit `bounces`
 *       R = R + L                                            (per channel, one f32 add, all four channels)
 *   radiance[i] = R
 *
 * Everything else of per_pixel is exactly as in a frame: the three-draw jitter
 * d += (2r-1)*0.0005 is not renormalised; the material clamp, the sRGB table, the texture
 * clamps and the environment lookup are unchanged; so are the glass, specular and diffuse
 * decisions and their draw order. Every value is bit-identical to the reference's arithmetic.
 * Consequences:
 *  - The result is the accumulation one rt_compute_frame would produce for a pixel whose index
 *    is `stream`, whose cached direction is d and whose camera origin is o, starting from a
 *    zeroed accumulation with accumulate = 1, compute_per_frame = samples and
 *    accumulation_index = first_sample.
 *  - The caller divides by `samples`. Nothing is clamped or packed.
 *  - bounces == 0 gives all-zero radiance (the loop does not run) and is RT_OK.
 *    samples == 0 is RT_E_INVALID (whatever `count` is).
 *  - *segments receives the batch's counted ray segments under the rule of rt_ray_count: every
 *    trace_ray call is counted, and a path that escapes stops counting. In the device variant
 *    the kernel adds the batch's total into the caller's u64 (it is added to, not set: one
 *    reduction and one atomic add per wave at exit, not one per ray).
 *  - Exactness holds for the domain of the ray queries above, for every segment of a path:
 *    finite components, |direction| in [1e-5, 1e5], |origin| <= 1e15. Outside it the result is
 *    unspecified. Termination: each walk ends as a ray query's does (the
 *    walks' skip links only advance), and a lane runs at most samples * bounces walks.
 *
 * Scene visibility and side effects are those of rt_trace_rays: the query sees the scene as
 * of the call -- materials, textures and the environment map now matter too -- with the
 * accelerators prepared exactly as a dispatch prepares them, and changes nothing a render can
 * observe (queued frames stay queued; the accumulation, the output, the accumulation index,
 * rt_ray_count, the timing totals, the tile schedule, the feature planes and the denoiser's
 * buffers are untouched). The result does not depend on the brute-force mode, on any
 * rt_set_tuning key or on triangle pruning modes 0 and 1 (mode 2 is inexact here as for
 * frames and ray queries). It works on rank contexts (world_size > 1) as the other queries do.
 *
 * rt_radiance: host pointers, synchronous. Staged through the pinned buffer of rt_trace_rays
 * in chunks of tuning "query_chunk" rays (32 bytes in, 16 bytes out per ray). `segments` may
 * be NULL.
 * rt_radiance_device: device pointers on the context's device; rays and radiance 16-byte
 * aligned, segments_device (may be NULL) 8-byte aligned; stream-ordered on rt_stream(ctx), no
 * host copy, asynchronous. RT_E_INVALID when any of them is not device memory of the context's
 * device, as for rt_trace_rays_device.
 * Tuning "query_lds_mode" selects the scene placement as for the ray queries; by default
 * batches of fewer than 262144 walks (count * samples) read the scene from global memory.
 * count == 0 returns RT_OK and launches nothing; a NULL rays or radiance pointer with
 * count > 0 is RT_E_INVALID. */
RT_API int rt_radiance(rt_ctx* ctx, const rt_radiance_ray* rays, float* radiance /* 4 floats per ray */,
                       uint64_t count, uint32_t bounces, uint32_t first_sample, uint32_t samples,
                       uint64_t* segments /* may be NULL */);
RT_API int rt_radiance_device(rt_ctx* ctx, const void* rays_device, void* radiance_device, uint64_t count,
                              uint32_t bounces, uint32_t first_sample, uint32_t samples,
                              void* segments_device /* may be NULL; one u64, added to */);

/* ---- gather queries (ABI 12, additive: gather queries) ----------------------
 *
 * "How much light does this surface point gather?": per point, the summed light of `samples`
 * paths that leave the point through the renderer's own diffuse lobe. Irradiance probes and
 * lightmap texels: a few thousand to a million points with hundreds of hemisphere samples
 * each. The directions are drawn on the device with the reference's RNG, the samples of a point
 * are spread over the lanes of the device, and the reduction order is stated, so every value is
 * bit-exact and independent of placement and schedule.
 *
 * What comes back is what a roughness-1, non-specular, non-glass surface at the point would
 * gather in per_pixel (compute_shader.wgsl:210-314): the scatter direction there,
 * specular + (diffuse - specular) * roughness, is at roughness 1 the diffuse lobe's draw
 * normalize(n + (gx, gy, gz)) that step 2 below makes, to within the two roundings of that
 * lerp. A bake therefore matches the frames the same library renders. */

/* {position, stream}, {normal, pad}: the layout of rt_radiance_ray. 32 bytes. */
typedef struct rt_gather_point {
    float position[3];
    uint32_t stream;  /* takes the place of the pixel index in the seeds; use streams >= 1 */
    float normal[3];  /* used as given: not normalised */
    float _pad1;      /* ignored */
} rt_gather_point;

#if defined(__cplusplus)
static_assert(sizeof(rt_gather_point) == 32, "rt_gather_point is 32 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_gather_point) == 32, "rt_gather_point is 32 bytes");
#endif

/* Writes four floats per point, in order; nothing outside [0, 4 * count) is written.
 *
 * THE GATHER CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
 * written order, with no contraction. For point i with record (x, stream, n):
 *  1. Sample index and origin. For s = 0 .. samples-1, u = first_sample + s (u32, wrapping).
 *     o = x + n * 0.0001f per component: one multiply and one add (the reference's bounce
 *     offset, as restated at oracle/pathtrace_oracle.c:511).
 *  2. Direction. dseed = (stream * u * 326624u) ^ 0x9E3779B9u (u32, wrapping).
 *     gx, gy, gz = normal_distribution(&dseed) three times, in that order
 *     (compute_shader.wgsl:622-628, theta drawn before rho).
 *     dir = normalize(n + (gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and
 *     dot(v, v) = (x*x + y*y) + z*z. n is used as given and is not normalised.
 *  3. Path. L_s is the result rt_radiance defines for the record (o, stream, dir) with
 *     first_sample = u, samples = 1 and the call's bounces: per_pixel with its own seed
 *     stream * u * 326624u, its own jitter, and everything else of a frame.
 *  4. Reduction. P_j (j = 0 .. 63) starts at +0.0f on all four channels. For s ascending,
 *     P_{s mod 64} = P_{s mod 64} + L_s. Then, for off = 32, 16, 8, 4, 2, 1:
 *     P_j = P_j + P_{j+off} for every j < off. radiance[i] = P_0. Lanes that got no sample
 *     take part with +0.0f. (An xor butterfly gives the same bits on finite values, because
 *     f32 addition commutes.)
 * End of the gather contract.
 *
 * Consequences:
 *  - The caller divides by `samples`. Nothing is clamped or packed.
 *  - bounces == 0 gives all-zero radiance and no segments, and is RT_OK. samples == 0 is
 *    RT_E_INVALID (whatever `count` is).
 *  - Stream 0 makes both seeds constant, so it draws the same sample every time, as pixel 0
 *    does in the reference: callers use streams >= 1.
 *  - A draw of exactly 0 makes rho infinite, as in the reference; the result is then
 *    unspecified.
 *  - Exactness holds for the domain of the radiance queries, for every segment of a path
 *    (position and normal are such that o and dir are in it). Termination is theirs too: a lane
 *    runs at most ceil(samples / 64) * bounces walks per (point, stripe) it takes.
 *  - *segments receives the call's counted ray segments under the rule of rt_radiance: every
 *    trace_ray call is counted, and a path that escapes stops counting. In the device variant
 *    the kernel adds the total into the caller's u64 (it is added to, not set: one reduction
 *    and one atomic add per wave at exit).
 *
 * Scene visibility and side effects are those of rt_trace_rays: the query sees the scene as
 * of the call -- materials, textures and the environment map now matter too -- with the
 * accelerators prepared exactly as a dispatch prepares them, and changes nothing a render can
 * observe (queued frames stay queued; the accumulation, the output, the accumulation index,
 * rt_ray_count, the timing totals, the tile schedule, the feature planes and the denoiser's
 * buffers are untouched). The result does not depend on the brute-force mode, on any
 * rt_set_tuning key or on triangle pruning modes 0 and 1 (mode 2 is inexact here as for
 * frames and ray queries). It works on rank contexts (world_size > 1) as the other queries do.
 *
 * Both entry points run in launches of at most tuning "gather_chunk" points: the partials
 * P_j of a launch live in a buffer the context owns, 1 KB per point (16 MB at the default),
 * allocated on first use and freed by rt_destroy.
 * rt_gather: host pointers, synchronous. Staged through the pinned buffer of rt_trace_rays
 * in chunks of tuning "query_chunk" points (32 bytes in, 16 bytes out per point). `segments`
 * may be NULL.
 * rt_gather_device: device pointers on the context's device; points and radiance 16-byte
 * aligned, segments_device (may be NULL) 8-byte aligned; stream-ordered on rt_stream(ctx), no
 * host copy, asynchronous. RT_E_INVALID when any of them is not device memory of the context's
 * device, as for rt_trace_rays_device.
 * Tuning "query_lds_mode" selects the scene placement as for the ray queries; by default
 * calls of fewer than 262144 walks (count * samples) read the scene from global memory.
 * count == 0 returns RT_OK and launches nothing; a NULL points or radiance pointer with
 * count > 0 is RT_E_INVALID. */
RT_API int rt_gather(rt_ctx* ctx, const rt_gather_point* points, float* radiance /* 4 floats per point */,
                     uint64_t count, uint32_t bounces, uint32_t first_sample, uint32_t samples,
                     uint64_t* segments /* may be NULL */);
RT_API int rt_gather_device(rt_ctx* ctx, const void* points_device, void* radiance_device, uint64_t count,
                            uint32_t bounces, uint32_t first_sample, uint32_t samples,
                            void* segments_device /* may be NULL; one u64, added to */);

/* ---- probe queries (ABI 12, additive: probe queries) ------------------------
 *
 * "What light arrives at this point in free space, from every direction?": per probe, the
 * projection of the incoming light onto the nine second-order spherical harmonics, per colour
 * channel, from `samples` paths that leave the point in uniform directions. Irradiance and
 * reflection probes for dynamic objects, which look the probe up with whatever normal they have
 * at the time: a few to a few thousand probes with hundreds to thousands of samples each. The
 * directions are drawn on the device with the reference's RNG, every (probe, sample) path is a
 * work item of its own, and the reduction order is stated, so every value is bit-exact and
 * independent of placement and schedule. */

/* {position, stream}: one 16-byte load. */
typedef struct rt_probe {
    float position[3];
    uint32_t stream;  /* takes the place of the pixel index in the seeds; use streams >= 1 */
} rt_probe;

#if defined(__cplusplus)
static_assert(sizeof(rt_probe) == 16, "rt_probe is 16 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_probe) == 16, "rt_probe is 16 bytes");
#endif

/* Writes 36 floats per probe, in order: coefficient k = 0 .. 8 at floats [4k, 4k + 4) as rgba;
 * nothing outside [0, 36 * count) is written.
 *
 * THE PROBE CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
 * written order, with no contraction. For probe i with record (x, stream):
 *  1. Sample index. For s = 0 .. samples-1, u = first_sample + s (u32, wrapping).
 *  2. Direction. dseed = (stream * u * 326624u) ^ 0x9E3779B9u (u32, wrapping).
 *     gx, gy, gz = normal_distribution(&dseed) three times, in that order
 *     (compute_shader.wgsl:622-628, theta drawn before rho).
 *     dir = normalize((gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and
 *     dot(v, v) = (x*x + y*y) + z*z: a uniform direction on the sphere.
 *  3. Path. L_s is the result rt_radiance defines for the record (x, stream, dir) with
 *     first_sample = u, samples = 1 and the call's bounces. The origin is x as given (no offset).
 *  4. Basis, on dir = (dx, dy, dz) of step 2 (before per_pixel's jitter):
 *     b0 = 0.28209479f                       b1 = 0.48860251f * dy
 *     b2 = 0.48860251f * dz                  b3 = 0.48860251f * dx
 *     b4 = 1.09254843f * (dx*dy)             b5 = 1.09254843f * (dy*dz)
 *     b6 = 0.31539157f * (3.0f*(dz*dz) - 1.0f)
 *     b7 = 1.09254843f * (dx*dz)             b8 = 0.54627422f * (dx*dx - dy*dy)
 *     T_{s,k} = L_s * b_k: one multiply per channel, all four channels.
 *  5. Reduction, for each k = 0 .. 8 on its own: P_j (j = 0 .. 63) starts at +0.0f. For s ascending,
 *     P_{s mod 64} = P_{s mod 64} + T_{s,k}. Then, for off = 32, 16, 8, 4, 2, 1:
 *     P_j = P_j + P_{j+off} for every j < off. sh[i][k] = P_0. Lanes that got no sample take part
 *     with +0.0f.
 * End of the probe contract.
 *
 * Consequences:
 *  - The caller multiplies by 4 pi / `samples` to get the radiance coefficients (the directions
 *    are uniform, with density 1 / 4 pi). Nothing is clamped.
 *  - bounces == 0 gives all-zero coefficients and no segments, and is RT_OK. samples == 0 is
 *    RT_E_INVALID (whatever `count` is), and so is `samples` above 16777216: one probe's
 *    scratch is then 256 MB, the most the call will allocate.
 *  - Stream 0 makes both seeds constant, so it draws the same sample every time: callers use
 *    streams >= 1.
 *  - A draw of exactly 0 makes rho infinite, as in the reference; the result is then
 *    unspecified.
 *  - Where no drawn component gx, gy, gz is +-0, a probe's L_s is bit for bit the L_s of a gather
 *    point at x with normal (0, 0, 0) (rt_gather's steps 1 to 3 with n = 0).
 *  - The exactness domain and the termination argument are those of the radiance queries: a
 *    lane runs at most `bounces` walks per (probe, sample) it takes.
 *  - *segments receives the call's counted ray segments under the rule of rt_radiance; in the
 *    device variant the kernel adds the total into the caller's u64 (added to, not set).
 *
 * Scene visibility and side effects are those of rt_gather: the query sees the scene as of the
 * call and changes nothing a render can observe. It works on rank contexts (world_size > 1).
 *
 * Both entry points run in launches of at most tuning "probe_chunk" paths, but of whole probes:
 * max(1, probe_chunk / samples) probes per launch. The lights L_s of a launch live in a buffer
 * the context owns, 16 bytes per path (16 MB at the default), allocated on first use and freed by
 * rt_destroy. A call of more than one launch keeps two in flight, on the context's two streams,
 * each with its own half of a buffer of twice that size (32 MB at the default), where that stays
 * within 256 MB; rt_stream(ctx) is ordered after both before the call returns.
 * rt_probe_sh: host pointers, synchronous. Staged through the pinned buffer of rt_trace_rays
 * in chunks of tuning "query_chunk" probes (16 bytes in, 144 bytes out per probe). `segments`
 * may be NULL.
 * rt_probe_sh_device: device pointers on the context's device; probes and sh 16-byte aligned,
 * segments_device (may be NULL) 8-byte aligned; stream-ordered on rt_stream(ctx), no host copy,
 * asynchronous. RT_E_INVALID when any of them is not device memory of the context's device, as
 * for rt_gather_device.
 * Tuning "query_lds_mode" selects the scene placement as for the ray queries; by default
 * calls of fewer than 262144 walks (count * samples) read the scene from global memory.
 * count == 0 returns RT_OK and launches nothing; a NULL probes or sh pointer with count > 0 is
 * RT_E_INVALID. */
RT_API int rt_probe_sh(rt_ctx* ctx, const rt_probe* probes, float* sh /* 36 floats per probe: 9 x rgba */,
                       uint64_t count, uint32_t bounces, uint32_t first_sample, uint32_t samples,
                       uint64_t* segments /* may be NULL */);
RT_API int rt_probe_sh_device(rt_ctx* ctx, const void* probes_device, void* sh_device, uint64_t count,
                              uint32_t bounces, uint32_t first_sample, uint32_t samples,
                              void* segments_device /* may be NULL; one u64, added to */);

/* ---- ambient queries (ABI 12, additive: ambient queries) ---------------------
 *
 * "Which part of the hemisphere over this surface point is open?": per point, the number of
 * `samples` directions through the gather's lobe that nothing blocks within t_max (ambient
 * occlusion, or sky visibility for an unbounded t_max) and the sum of those directions (the bent
 * normal). Occlusion baking for lightmap texels and vertices: the any-hit counterpart of
 * rt_gather. The directions are drawn on the device, every sample is one any-hit search of
 * rt_occluded, the samples of a point are spread over the lanes of the device, and the reduction
 * order is stated, so every value is bit-exact and independent of placement and schedule. The
 * bent normal is also the direction to look an rt_probe_sh probe up with. */

/* {position, stream}, {normal, t_max}: the layout of rt_gather_point with the distance bound in the
 * place of _pad1 (where rt_occlusion_ray keeps it). 32 bytes. */
typedef struct rt_ambient_point {
    float position[3];
    uint32_t stream;  /* as in rt_gather_point; use streams >= 1 */
    float normal[3];  /* used as given: not normalised */
    float t_max;      /* the AO radius, in world units (the directions are unit length) */
} rt_ambient_point;

#if defined(__cplusplus)
static_assert(sizeof(rt_ambient_point) == 32, "rt_ambient_point is 32 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_ambient_point) == 32, "rt_ambient_point is 32 bytes");
#endif

/* Writes four floats per point, in order: bent.x, bent.y, bent.z, open; nothing outside
 * [0, 4 * count) is written.
 *
 * THE AMBIENT CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
 * written order, with no contraction. For point i with record (x, stream, n, t_max):
 *  1. Sample index and origin: step 1 of the gather contract. For s = 0 .. samples-1,
 *     u = first_sample + s (u32, wrapping). o = x + n * 0.0001f per component: one multiply and
 *     one add.
 *  2. Direction: step 2 of the gather contract. dseed = (stream * u * 326624u) ^ 0x9E3779B9u
 *     (u32, wrapping). gx, gy, gz = normal_distribution(&dseed) three times, in that order.
 *     dir = normalize(n + (gx, gy, gz)) with normalize(v) = v * (1.0f / sqrt(dot(v, v))) and
 *     dot(v, v) = (x*x + y*y) + z*z. n is used as given and is not normalised. There is no
 *     jitter: dir is the ray's direction as is.
 *  3. Visibility. B_s is the byte rt_occluded defines for the record (o, dir, t_max): 1 iff a
 *     primitive is accepted at a non-NaN distance t < t_max (strictly); t_max <= 0 or NaN
 *     gives 0. V_s = 1 - B_s.
 *  4. Term. T_s = (dir.x, dir.y, dir.z, 1.0f) where V_s == 1, and
 *     T_s = (+0.0f, +0.0f, +0.0f, +0.0f) where V_s == 0.
 *  5. Reduction: step 4 of the gather contract on T_s. P_j (j = 0 .. 63) starts at +0.0f on all
 *     four channels. For s ascending, P_{s mod 64} = P_{s mod 64} + T_s. Then, for
 *     off = 32, 16, 8, 4, 2, 1: P_j = P_j + P_{j+off} for every j < off. out[i] = P_0. Lanes
 *     that got no sample take part with +0.0f.
 * End of the ambient contract.
 *
 * Consequences:
 *  - `open` (channel w) is an integer-valued float, exact whatever the order of addition, because
 *    samples <= 16777216. Above that the call is RT_E_INVALID.
 *  - samples == 0 is RT_E_INVALID (whatever `count` is).
 *  - Ambient occlusion is open / samples. The bent normal is `bent`, normalised by the caller;
 *    `bent` is all +0.0f when open == 0.
 *  - t_max = +inf or 3.4028235e38f asks for sky visibility: any hit at all, as rt_occluded
 *    defines it.
 *  - t_max <= 0 or NaN gives open == samples (and `bent` the reduction of every direction).
 *  - Stream 0 makes the seed constant, so it draws the same direction every time, and a draw of
 *    exactly 0 makes rho infinite (the result is then unspecified): the caveats of rt_gather.
 *  - The exactness domain and the termination argument are those of the occlusion queries
 *    (position and normal are such that o and dir are in it). A lane runs at most
 *    ceil(samples / 64) searches per (point, stripe) it takes.
 *
 * Scene visibility and side effects are those of rt_occluded: the query sees the scene as of
 * the call; materials, textures and the environment do not matter; queued frames stay queued and
 * nothing a render observes changes. The result does not depend on the brute-force mode, on any
 * rt_set_tuning key or on triangle pruning modes 0 and 1. It works on rank contexts
 * (world_size > 1).
 *
 * Both entry points run in launches of at most tuning "gather_chunk" points, with the partials
 * P_j in the buffer rt_gather uses (1 KB per point of a launch).
 * rt_ambient: host pointers, synchronous. Staged through the pinned buffer of rt_trace_rays in
 * chunks of tuning "query_chunk" points (32 bytes in, 16 bytes out per point).
 * rt_ambient_device: device pointers on the context's device; points and out 16-byte aligned;
 * stream-ordered on rt_stream(ctx), no host copy, asynchronous. RT_E_INVALID when either is not
 * device memory of the context's device, as for rt_gather_device.
 * Tuning "query_lds_mode" selects the scene placement as for the ray queries; by default calls
 * of fewer than 262144 walks (count * samples) read the scene from global memory.
 * count == 0 returns RT_OK and launches nothing; a NULL points or out pointer with count > 0 is
 * RT_E_INVALID. */
RT_API int rt_ambient(rt_ctx* ctx, const rt_ambient_point* points, float* out /* 4 floats per point */,
                      uint64_t count, uint32_t first_sample, uint32_t samples);
RT_API int rt_ambient_device(rt_ctx* ctx, const void* points_device, void* out_device, uint64_t count,
                             uint32_t first_sample, uint32_t samples);

/* ---- lens queries (ABI 12, additive: lens queries) ---------------------------
 *
 * "What does this camera see?" for cameras other than the context's pinhole: a thin lens (depth
 * of field), an orthographic view, and an equirectangular panorama captured at a point (which
 * rt_upload_env_map takes back as a reflection probe). The rays are drawn on the device from a
 * 176-byte descriptor, a lens sample per (pixel, sample index), so no records cross the bus: a
 * radiance query of the same rays needs one 32-byte rt_radiance_ray per pixel per sample. The
 * image width x height belongs to the descriptor, not to the context's framebuffer; nothing of
 * the framebuffer is read or written. */

#define RT_LENS_PERSPECTIVE  0u
#define RT_LENS_ORTHOGRAPHIC 1u
#define RT_LENS_EQUIRECT     2u

typedef struct rt_lens_camera {
    float inverse_projection[16]; /* column-major, glam layout; PERSPECTIVE only */
    float inverse_view[16];       /* column-major; used as a rotation only (w = 0); EQUIRECT ignores it */
    float origin[3];
    float aspect;                 /* the factor camera_ray multiplies nx by: f32(width)/f32(height) in a frame */
    uint32_t kind;                /* RT_LENS_* */
    uint32_t width, height;       /* the image the pixel indices refer to; width * height <= 2^32 */
    uint32_t stream_base;         /* pixel i draws from the RNG stream stream_base + i */
    float aperture;               /* lens radius in view units; 0 = pinhole; PERSPECTIVE only */
    float focus;                  /* distance of the focal plane along the view axis, > 0 when aperture > 0 */
    float ortho_half_height;      /* ORTHOGRAPHIC: half the view volume's height, > 0 */
    float _pad;                   /* ignored */
} rt_lens_camera;

#if defined(__cplusplus)
static_assert(sizeof(rt_lens_camera) == 176, "rt_lens_camera is 176 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_lens_camera) == 176, "rt_lens_camera is 176 bytes");
#endif

/* Items are the pixels first_pixel .. first_pixel + count - 1 of the descriptor's image in
 * row-major order (pixel i = y*width + x); the caller tiles by ranges. rt_lens writes four floats
 * per pixel of the range, in order; nothing outside [0, 4 * count) is written.
 *
 * THE LENS CONTRACT. Everything is f32. Each written operation is one IEEE operation, in the
 * written order, with no contraction. For pixel index i = y*width + x of the descriptor's image,
 * stream = stream_base + i (u32, wrapping) and sample index u:
 *  A. Screen point, as in camera_ray. xc = f32(x)/f32(width), yc = f32(y)/f32(height).
 *     nx = xc*2.0f - 1.0f, ny = yc*2.0f - 1.0f, ax = nx*aspect.
 *  B. PERSPECTIVE. t = P^-1 * (ax, ny, 1, 1) with glam's Mat4 * Vec4 =
 *     ((c0*x + c1*y) + c2*z) + c3*w per component (P^-1 = inverse_projection, V^-1 = inverse_view).
 *     ws = normalize(t.xyz / t.w) with normalize(v) = v * (1.0f / sqrt((x*x + y*y) + z*z)).
 *     If aperture == 0: o = origin, d = (V^-1 * (ws, 0)).xyz: the very bits of camera_ray.
 *     Otherwise: lseed = (stream * u * 326624u) ^ 0x85EBCA6Bu (u32, wrapping).
 *     r1 = random(&lseed), r2 = random(&lseed), in that order (compute_shader.wgsl:587-599).
 *     rad = aperture * sqrt(r1), th = 6.2831850051879883f * r2.
 *     lx = rad * cos(th), ly = rad * cos(th - 1.5707963705062866f).
 *     k = focus / (0.0f - ws.z), f = ws * k.
 *     dv = normalize((f.x - lx, f.y - ly, f.z)), d = (V^-1 * (dv, 0)).xyz.
 *     o = origin + (V^-1 * (lx, ly, 0, 0)).xyz.
 *     cos is the oracle's oracle_cosf (cosf_c on the device; its arguments stay within
 *     |x| <= 2 pi) and sqrt is correctly rounded.
 *  C. ORTHOGRAPHIC. o = origin + (V^-1 * (ax*ortho_half_height, ny*ortho_half_height, 0, 0)).xyz.
 *     d = (V^-1 * (0, 0, -1, 0)).xyz.
 *  D. EQUIRECT. The inverse of environment_map_coords at pixel centres, world-aligned.
 *     uc = (f32(x) + 0.5f)/f32(width), vc = (f32(y) + 0.5f)/f32(height).
 *     az = (uc - 0.5f) * (2.0f*WGSL_PI), el = (vc - 0.5f) * WGSL_PI, ce = cos(el), with
 *     WGSL_PI = 3.1415926536f.
 *     d = (ce*cos(az), cos(el - 1.5707963705062866f), ce*cos(az - 1.5707963705062866f)). o = origin.
 *  E. Path and sum. R = +0.0f on all four channels. For s = 0 .. samples-1 ascending,
 *     u = first_sample + s (u32, wrapping); L_s is the result rt_radiance defines for the record
 *     (o, stream, d) of step B, C or D at u with first_sample = u, samples = 1 and the call's
 *     bounces, per_pixel's own jitter included. R = R + L_s per channel. radiance[i] = R.
 * End of the lens contract.
 *
 * rt_lens_rays writes the rt_radiance_ray (o, stream, d, +0.0f) of steps A to D for
 * u = sample_index, one per pixel of the range, in order.
 *
 * Consequences:
 *  1. The pinhole case reproduces the frame: PERSPECTIVE with aperture == 0, stream_base == 0 and
 *     the context's size, matrices (rt_update_camera_matrices), aspect and origin gives the
 *     accumulation that `samples` frames from accumulation_index = first_sample leave in a zeroed
 *     buffer, bit for bit.
 *  2. rt_radiance on the records of rt_lens_rays(.., u) with first_sample = u, samples = 1 equals
 *     rt_lens with first_sample = u, samples = 1.
 *  3. bounces == 0 gives all-zero radiance and no segments, and is RT_OK. samples == 0 is
 *     RT_E_INVALID (whatever `count` is). The caller divides by `samples`; nothing is clamped.
 *  4. A pixel whose stream is 0 repeats its lens point (and its path) for every u, as pixel 0
 *     repeats its seed in the reference: callers use stream_base >= 1 unless they want
 *     consequence 1.
 *  5. A draw of r1 == 0 gives the lens centre.
 *  6. RT_E_INVALID for: an unknown kind; width or height 0; width * height > 2^32; a range
 *     outside the image (first_pixel + count > width * height); aperture negative or not finite;
 *     focus <= 0 (or NaN) with aperture > 0; ortho_half_height <= 0 (or NaN) for ORTHOGRAPHIC; a
 *     NULL cam, radiance or rays pointer with count > 0; device pointers that are not device
 *     memory of the context's device, or not aligned: 16 bytes for rays and radiance, 8 for
 *     segments. count == 0 returns RT_OK and launches nothing.
 *  7. Scene visibility, side effects (none a render can observe: queued frames stay queued),
 *     independence of the brute-force mode and of every rt_set_tuning key, rank contexts, the
 *     exactness domain and the counted segments are those of rt_radiance, for the rays of steps
 *     B to D.
 *
 * `cam` is host memory in all four entry points and is read before the call returns.
 * rt_lens, rt_lens_rays: host result pointers, synchronous; the range runs in chunks of tuning
 * "query_chunk" pixels through the pinned buffer of rt_trace_rays (16 or 32 bytes out per pixel,
 * nothing in). `segments` may be NULL.
 * rt_lens_device, rt_lens_rays_device: device result pointers on the context's device;
 * stream-ordered on rt_stream(ctx), no host copy, asynchronous; segments_device (may be NULL) is
 * added to, not set.
 * Tuning "query_lds_mode" selects the scene placement as for the ray queries; by default calls of
 * fewer than 262144 walks (count * samples) read the scene from global memory. */
RT_API int rt_lens(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count,
                   float* radiance /* 4 floats per pixel */, uint32_t bounces, uint32_t first_sample,
                   uint32_t samples, uint64_t* segments /* may be NULL */);
RT_API int rt_lens_device(rt_ctx* ctx, const rt_lens_camera* cam /* host memory */, uint64_t first_pixel,
                          uint64_t count, void* radiance_device, uint32_t bounces, uint32_t first_sample,
                          uint32_t samples, void* segments_device /* may be NULL; one u64, added to */);
RT_API int rt_lens_rays(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count,
                        uint32_t sample_index, rt_radiance_ray* rays);
RT_API int rt_lens_rays_device(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count,
                               uint32_t sample_index, void* rays_device);

/* ---- feature buffers and the denoiser (ABI 12, additive: denoiser) ----------
 *
 * What an interactive host shows right after the camera or the scene moved: the reference resets
 * the accumulation on every edit and then displays a handful of samples per pixel. Two pieces:
 * the first-hit feature buffers (normal, depth, albedo: the "AOVs" a compositor or an external
 * denoiser also wants) and an edge-avoiding a-trous filter guided by them.
 *
 * FEATURES. Two float4 planes of width*height pixels, row-major:
 *   normal_depth: normal.xyz, t        albedo_hit: albedo.rgb, hit (1.0f or 0.0f)
 * Per pixel, the un-jittered camera ray exactly as rt_pick defines it and the record
 * rt_trace_rays returns for it. Hit: normal and t straight from the record; albedo is
 * sample_texture(materials[min(material_index, material_count-1)].texture_index, u, v).rgb with
 * the clamp, sRGB table and layer clamp of the path kernel's shading (compute_shader.wgsl:26-40);
 * emission is ignored. Miss: normal = 0, t = 3.4028235e38f, hit = 0, albedo = the environment
 * texel at environment_map_coords(direction) (compute_shader.wgsl:580-585). Every value is
 * bit-identical to the reference's arithmetic for that ray (exactness domain: the ray queries').
 * The planes depend only on camera, geometry, materials, textures and Params: the context keeps a
 * scene epoch that every rt_update_*, rt_upload_*, rt_update_camera*, rt_update_ray_directions,
 * rt_reset_accumulation, rt_set_object_models and rt_update_objects call bumps, and recomputes the
 * planes only when the epoch they were built at is stale. The frame is traced in bands of tuning
 * "feature_band" pixels (96 B of scratch per pixel of a band). Like a ray query, computing the
 * features changes nothing a render observes and leaves queued frames queued.
 *
 * rt_compute_features: asynchronous; a no-op when the planes are current.
 * rt_read_features: synchronous (computes the planes if stale); either pointer may be NULL; each
 *   receives width*height*4 floats.
 * rt_features_device: the planes' device pointers (computed if stale, stream-ordered on
 *   rt_stream(ctx)); valid until rt_destroy, rewritten by the next recomputation.
 *
 * THE ID PLANE. A third plane of width*height uint2, row-major, resolved from the same record as
 * the two planes above: id.x = rt_hit.kind and id.y = rt_hit.index (the object index of a triangle
 * hit, the sphere index as uploaded of a sphere hit); a miss is (0, 0). It is allocated with the
 * other planes and falls under the same scene-epoch rule.
 * rt_read_feature_ids: synchronous (computes the planes if stale); width*height*2 uint32.
 * rt_feature_ids_device: the plane's device pointer, like rt_features_device.
 *
 * THE FILTER. The arithmetic below is the contract.
 *
 * Everything is f32, one IEEE operation per written operation, in the written order.
 *
 * Inputs. Per pixel p:
 *   c0(p) = accumulation(p) / D, all four channels;
 *   D = (float)((k-1) * compute_per_frame);
 *   k is the context's accumulation counter, as reported by rt_accumulation_index;
 *   n(p), z(p), a(p), hit(p) from the feature planes.
 *
 * Host-side constants, computed in f32:
 *   N = (k-1)*compute_per_frame;
 *   s0 = sigma_color / sqrtf((float)N);
 *   k_a = 1.0f / (sigma_albedo*sigma_albedo);
 *   for iteration i: s_i = s0 * 0.5f^i (exact scaling) and k_c = 1.0f / (s_i*s_i).
 *
 * Iteration i = 0 .. iterations-1:
 *   step s = 1<<i;
 *   h = {1/16, 1/4, 3/8, 1/4, 1/16};
 *   taps q = p + s*(dx,dy);
 *   dy is the outer loop and dx the inner loop, each running -2..2 ascending.
 *
 * Centre tap. w = h[2]*h[2] (that is 9/64). It is always taken and evaluates no guide.
 *
 * Other taps. A tap is skipped (it adds nothing to either sum) if q is outside the image. Otherwise:
 *   Guide g:
 *     If hit(p) and hit(q) are both 0, then g = 1.
 *     If exactly one of them is 0, then g = 0.
 *     Otherwise g = wn*wz, with:
 *       d = max(0, (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z);
 *       wn = d^32, by five squarings;
 *       x = |z_p - z_q| / (sigma_depth*(z_p + z_q) + 1e-30f);
 *       wz = 1/(1 + x*x).
 *   Albedo:
 *     da = a_p - a_q;
 *     xa = ((da.r*da.r + da.g*da.g) + da.b*da.b) * k_a;
 *     ra = 1/(1+xa).
 *   Colour, on the current iteration's input:
 *     dc = c_p.rgb - c_q.rgb;
 *     xc = ((dc.r*dc.r + dc.g*dc.g) + dc.b*dc.b) * k_c;
 *     rc = 1/(1+xc).
 *   Weight: w = (((h[dy]*h[dx]) * g) * (ra*ra)) * (rc*rc).
 *   The tap is skipped unless w > 0. That test is false for NaN.
 *
 * Result per iteration. Per channel, num = num + w*c_q and den = den + w, in tap order starting
 * from 0. The result is num/den.
 *
 * After the last iteration the f32 RGBA result is kept. Its clamp01 then pack_to_u32 (the
 * truncating pack the frame output uses) goes to a separate denoised-output buffer.
 * iterations == 0 is just c0 and its pack. That pack equals rt_read_output of the same frame.
 * Pixels whose accumulation is not finite give unspecified values there only.
 *
 * The 1/sqrt(N) scaling narrows the colour weight as the accumulation converges: the filter
 * smooths hard at 1 sample per pixel and fades out as the noise does.
 *
 * rt_denoise is an observation point, like rt_copy_output_to_device: queued frames launch first,
 * then the features are computed if stale, then the filter runs, all stream-ordered on
 * rt_stream(ctx); asynchronous. It changes nothing a render observes: the accumulation,
 * rt_read_output, k, rt_ray_count, the timing totals and the tile schedule are untouched, and
 * rendering continues afterwards as if it had not been called. Its buffers (two colour planes, the
 * packed output, the feature planes and a band of scratch) are allocated on first use and freed by
 * rt_destroy. params == NULL: rt_denoise_default_params. Tuning "denoise_lds" selects how the
 * passes with step 1 and 2 read their taps (same bits either way).
 * RT_E_INVALID: no frame since the last reset (k-1 == 0, or N == 0); Params.accumulate != 1 (the accumulation
 * is never written then); iterations > 8; a sigma that is not finite or <= 0; a rank context
 * (world_size > 1).
 * rt_read_denoised: synchronous; the last rt_denoise's packed RGBA8 (width*height u32) and f32 RGBA
 *   (width*height*4 floats) results; either pointer may be NULL. RT_E_INVALID before any rt_denoise.
 * rt_copy_denoised_to_device: rt_copy_output_to_device for the packed denoised output, with the
 *   same arguments and errors; RT_E_INVALID before any rt_denoise. Asynchronous. */
typedef struct rt_denoise_params {
    uint32_t iterations;   /* a-trous iterations, 0..8 (step 1, 2, 4, ...) */
    float sigma_color;     /* colour tolerance at 1 sample per pixel */
    float sigma_albedo;
    float sigma_depth;     /* relative depth tolerance */
} rt_denoise_params;

#if defined(__cplusplus)
static_assert(sizeof(rt_denoise_params) == 16, "rt_denoise_params is 16 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_denoise_params) == 16, "rt_denoise_params is 16 bytes");
#endif

RT_API int rt_denoise_default_params(rt_denoise_params* out); /* {4, 1.0f, 0.1f, 0.05f} */
RT_API int rt_compute_features(rt_ctx* ctx);
RT_API int rt_read_features(rt_ctx* ctx, float* normal_depth, float* albedo_hit);
RT_API int rt_features_device(rt_ctx* ctx, const void** normal_depth, const void** albedo_hit);
RT_API int rt_read_feature_ids(rt_ctx* ctx, uint32_t* ids /* 2 per pixel: kind, index */);
RT_API int rt_feature_ids_device(rt_ctx* ctx, const void** ids);
RT_API int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params);
RT_API int rt_read_denoised(rt_ctx* ctx, uint32_t* rgba8_out, float* rgba_f32_out);
RT_API int rt_copy_denoised_to_device(rt_ctx* ctx, void* dst_device, uint32_t bytes_per_row);

/* ---- temporal reprojection for the denoiser (ABI 12, additive: temporal denoiser) ----
 *
 * While the camera keeps moving, every displayed frame is a fresh 1-spp estimate. rt_denoise_temporal
 * reprojects the previous call's blended result through the camera it was made with, validates it
 * against geometry (hit flag, normal, world position), blends it with the new samples weighted by a
 * per-pixel sample count, and then runs the a-trous filter with a colour tolerance that follows
 * that count. The filtered result lands in the denoised buffers that already exist: rt_read_denoised
 * and rt_copy_denoised_to_device serve it unchanged.
 *
 * STATE. Two history slots of three float4 planes each (96 B per pixel in all), allocated on the
 * first call and freed by rt_destroy. A slot holds C (rgba), X (xyz, hit), Nn (normal.xyz, n), the
 * matrix it was written with and a generation tag. The context keeps an accumulation generation G
 * that rt_reset_accumulation increments; nothing else increments it. A call at generation G chooses
 * the previous slot like this: if the current slot is valid and its tag is not G, the slots swap
 * roles (the old current becomes previous); if the current slot is valid and its tag equals G,
 * previous stays what it was (possibly none) and the current slot is overwritten. Within one
 * accumulation generation the history is therefore always the last result of the generation before
 * it -- the past is never counted twice -- and the growing accumulation outweighs it as N grows.
 * rt_temporal_reset invalidates both slots: call it after texture or lighting edits, and after a
 * material edit that is not marked RT_MOTION_DROP, which reprojection cannot validate. Object and
 * sphere motion no longer need a reset: rt_denoise_temporal_motion (below) follows them.
 *
 * world_to_pixel is the CURRENT camera's map from world space to pixel coordinates (pixel (x, y) is
 * where the un-jittered ray of pixel (x, y) lands); it is stored with the slot and used by the next
 * generation's call. It is an input to the contract, not part of it.
 *
 * THE TEMPORAL STAGE (rt_denoise_temporal; tests/temporal_ref.py restates it from here).
 *
 * Everything is f32, one IEEE operation per written operation, in the written order, with no
 * contraction and correctly rounded division. W and H are (float)width and (float)height.
 *
 * Per pixel p = (x, y):
 *
 * 1. Current estimate.
 *   c = accumulation(p) / D on all four channels;
 *   N = (float)((k-1)*compute_per_frame), exactly the c0 and N of rt_denoise (D is N);
 *   (o, d) is the pixel's un-jittered ray as rt_pick defines it;
 *   n_p, t_p and hit_p come from the feature planes.
 *
 * 2. World point.
 *   Hit: X_p = o + d*t_p per component (one multiply, one add), and wv = 1.
 *   Miss: X_p = d, and wv = 0.
 *
 * 3. Projection through the previous slot's matrix M. This step runs only if a previous slot exists.
 *   For rows i = 0, 1, 3: c_i = (M[i]*X.x + M[4+i]*X.y) + M[8+i]*X.z. On a hit, c_i = c_i + M[12+i] follows.
 *   There is no history unless c_3 > 0.
 *   fx = c_0/c_3 and fy = c_1/c_3.
 *   There is no history unless fx > -1 && fx < W && fy > -1 && fy < H. Every one of these tests is false for NaN.
 *
 * 4. Bilinear taps.
 *   x0 = floorf(fx), y0 = floorf(fy), ax = fx - x0, ay = fy - y0, bx = 1 - ax, by = 1 - ay.
 *   The taps q, in this order:
 *     (x0, y0) with w = bx*by;
 *     (x0+1, y0) with w = ax*by;
 *     (x0, y0+1) with w = bx*ay;
 *     (x0+1, y0+1) with w = ax*ay.
 *   A tap counts only if q is inside the image, w > 0, and hit_q == hit_p.
 *   On a hit, two further tests apply:
 *     the normal: (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z >= normal_min;
 *     the position: e2 <= (sigma_position*sigma_position) * r2, with
 *       e = X_p - X_q,
 *       e2 = (e.x*e.x + e.y*e.y) + e.z*e.z,
 *       f = X_p - o,
 *       r2 = (f.x*f.x + f.y*f.y) + f.z*f.z.
 *   Misses need nothing further.
 *
 * 5. History sums.
 *   sw = sw + w, hc = hc + w*C_q (per channel) and hn = hn + w*n_q, in tap order starting from 0.
 *   There is no history unless sw > 0.
 *   Otherwise h = hc/sw and nh = min(hn/sw, (float)max_history).
 *
 * 6. Blend.
 *   Without history: out = c and n_out = N.
 *   With history: tot = nh + N, a = N/tot, out = h + (c - h)*a per channel, and n_out = tot.
 *
 * 7. Store. The current slot gets C = out, X = (X_p, hit_p) and Nn = (n_p, n_out). Its matrix becomes
 *   params->world_to_pixel and its tag becomes G.
 *
 * 8. Filter. The a-trous iterations of rt_denoise run on c0 := out. The colour scale is per pixel:
 *   s_i = sigma_color * 0.5f^i (exact scaling);
 *   K_i = 1.0f/(s_i*s_i);
 *   k_c(p) = n_out(p) * K_i, using the centre pixel's count.
 *   Everything else is word for word the pass above. iterations == 0 gives out and its pack.
 *
 * Because k_c rounds differently (n_out*K_i here, 1/(s_i*s_i) with s0 = sigma_color/sqrtf(N) above), a
 * call without history is close to rt_denoise of the same frame but is not promised bit-equal.
 * End of the temporal contract.
 *
 * rt_denoise_temporal is an observation point exactly like rt_denoise: queued frames launch first,
 * then the features are computed if stale, then the temporal stage runs, then the filter, all
 * stream-ordered on rt_stream(ctx) and asynchronous. The accumulation, rt_read_output, k,
 * rt_ray_count, the timing totals, the tile schedule, the feature planes and a later plain
 * rt_denoise are all unaffected. denoise_params == NULL: rt_denoise_default_params.
 * Errors: those of rt_denoise, plus RT_E_INVALID for a NULL rt_temporal_params (the matrix has no
 * default), a non-finite matrix entry, max_history outside 1..65536, sigma_position not finite or
 * <= 0, normal_min not finite or outside [-1, 1]. A failing call leaves the history as it was.
 * rt_temporal_reset: drops all history; RT_OK when there is none. Needed after texture and lighting
 *   edits and after material edits not marked RT_MOTION_DROP; not after object or sphere motion
 *   that rt_denoise_temporal_motion is told about.
 * rt_read_temporal: synchronous; the pre-filter blend `out` (width*height*4 floats) and the per-pixel
 *   history length n_out (width*height floats) of the last call; either pointer may be NULL.
 *   RT_E_INVALID before any rt_denoise_temporal and after rt_temporal_reset. */
typedef struct rt_temporal_params {
    float world_to_pixel[16]; /* column-major 4x4, glam layout: the CURRENT camera's map from world space to
                                 pixel coordinates; rows 0, 1, 3 give x*w, y*w, w; row 2 is ignored */
    uint32_t max_history;     /* cap on the samples the past may weigh, 1..65536 */
    float sigma_position;     /* relative world-space tolerance */
    float normal_min;         /* minimum n_p . n_q, in [-1, 1] */
    uint32_t _reserved;       /* 0 */
} rt_temporal_params;

#if defined(__cplusplus)
static_assert(sizeof(rt_temporal_params) == 80, "rt_temporal_params is 80 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_temporal_params) == 80, "rt_temporal_params is 80 bytes");
#endif

RT_API int rt_temporal_default_params(rt_temporal_params* out); /* matrix all zero, {32, 0.02f, 0.9f, 0} */
RT_API int rt_denoise_temporal(rt_ctx* ctx, const rt_temporal_params* params,
                               const rt_denoise_params* denoise_params /* NULL: defaults */);
RT_API int rt_temporal_reset(rt_ctx* ctx);
RT_API int rt_read_temporal(rt_ctx* ctx, float* rgba /* W*H*4 */, float* history /* W*H */);

/* ---- the display transform (ABI 12, additive: display transform) ------------------------
 *
 * Radiance to display codes on the device. The frame output, rt_denoise and rt_denoise_temporal all
 * finish with clamp01 and the truncating pack (the reference's pack_to_u32): with emitters far above
 * 1 much of a frame lands at 255. rt_display meters the source, adapts an exposure over time, applies
 * a tone curve and optionally encodes to sRGB, stream-ordered and with no host round trip. The
 * reference's look stays the default everywhere else.
 *
 * THE DISPLAY CONTRACT (tests/display_ref.py restates it from here).
 *
 * Everything is f32 unless marked integer. Each written operation is one IEEE operation, in the
 * written order, with no contraction and correctly rounded division. No exp, log or pow is used.
 *
 * S(p) is the source pixel, with four channels: accumulation(p) / D on all four channels (exactly
 * rt_denoise's c0) for RT_DISPLAY_ACCUMULATION, the f32 result of the last denoise call for
 * RT_DISPLAY_DENOISED, the caller's plane for RT_DISPLAY_PLANE.
 *
 * 1. Metering (only when auto_exposure == 1).
 *   Per pixel, L = (0.2126f*S.r + 0.7152f*S.g) + 0.0722f*S.b.
 *   The pixel is metered iff L > 0 && L < +inf. Both tests are false for NaN.
 *   Its bin is an integer: j = clamp((int)(bits(L) >> 20) - 888, 0, 255).
 *     This gives 8 bins per octave over [2^-16, 2^16). 888 = (127-16)*8.
 *     Smaller values go to bin 0, larger ones to bin 255.
 *   hist[j] += 1.
 *   The histogram is a set of integer counts, so it is independent of schedule and order.
 *
 * 2. Exposure solve (integer until the last line; u64).
 *   total = sum of hist.
 *   lo = total*low_permille/1000.
 *   hi = total - total*high_permille/1000.
 *   Walking j ascending with a running sum cum, n_j = |[cum, cum+hist[j]) intersected with [lo, hi)|.
 *   Nn = sum of n_j and Sn = sum of n_j*(2j+1).
 *   If total == 0: there is no target.
 *   Otherwise:
 *     a = (2*Sn + Nn) / (2*Nn). This is the mean bin centre in 1/16 octaves, rounded. It is in 1..511.
 *     n = 256 - a, q = floor(n / 16), r = n - 16*q.
 *     E_t = key * ldexpf(T16[r], q).
 *     E_t = min(max(E_t, min_exposure), max_exposure).
 *   T16[r] is 2^(r/16) rounded to f32. Its bits are:
 *     0x3f800000, 0x3f85aac3, 0x3f8b95c2, 0x3f91c3d3, 0x3f9837f0, 0x3f9ef532, 0x3fa5fed7, 0x3fad583f,
 *     0x3fb504f3, 0x3fbd08a4, 0x3fc5672a, 0x3fce248c, 0x3fd744fd, 0x3fe0ccdf, 0x3feac0c7, 0x3ff5257d.
 *
 * 3. Adaptation. E_prev is the state.
 *   State none, target none: E = min(max(1.0f, min_exposure), max_exposure).
 *   State none, target E_t: E = E_t.
 *   State E_prev, target none: E = E_prev.
 *   State E_prev, target E_t: E = E_prev + (E_t - E_prev)*adaptation.
 *   The state becomes E.
 *   With auto_exposure == 0: E = params.exposure. The state and the stored histogram are left untouched.
 *
 * 4. Tone curve, per colour channel.
 *   x = S.c * E.
 *   x = x > 0 ? x : 0. NaN and -0 give +0.
 *   x = min(x, 65536.0f).
 *   LINEAR: y = x.
 *   REINHARD: iw2 = 1.0f/(white*white), computed on the host in f32; y = (x*(1.0f + x*iw2)) / (1.0f + x).
 *   ACES: y = (x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f).
 *   Then y = min(y, 1.0f).
 *   Alpha is clamp01(S.a) with no exposure and no curve (NaN gives 0, as in the frame's clamp). It is
 *   always packed as the frame packs it.
 *
 * 5. Encode.
 *   NONE: code = (uint32_t)(y*255.0f) & 0xff, which is pack_rgba8.
 *   SRGB: code is the largest j in 0..255 with srgb_table[j] <= y.
 *     The table is the 256-entry table of rt_srgb_table.
 *     It is strictly increasing, so a branch-free 8-step search finds j.
 *   The packed word is r | g<<8 | b<<16 | a<<24.
 * End of the display contract.
 *
 * Consequences:
 *  - With auto_exposure = 0, exposure = 1, RT_TONE_LINEAR and RT_ENCODE_NONE the display equals
 *    rt_read_output of the same frame for RT_DISPLAY_ACCUMULATION, and the packed result of
 *    rt_read_denoised for RT_DISPLAY_DENOISED.
 *  - Exposure resolution is 1/16 stop.
 *  - The SRGB encode is the exact inverse of the texture decode: encode(srgb_table[j]) == j.
 *
 * rt_display is an observation point exactly like rt_denoise. For RT_DISPLAY_ACCUMULATION queued
 * frames launch first; the other sources leave them queued. Everything is stream-ordered on
 * rt_stream(ctx) and asynchronous; there is no host synchronisation anywhere in it: the adapted
 * exposure lives in device memory and is consumed there. It changes nothing that a render, a query,
 * rt_denoise or rt_denoise_temporal observes: the accumulation, the output, k, rt_ray_count, the
 * timing totals, the tile schedule, the feature planes, the denoised buffers and the temporal history
 * are untouched. It does not run the denoiser: RT_DISPLAY_DENOISED reads what the last rt_denoise or
 * rt_denoise_temporal left. Its buffers (one packed u32 plane, 256 live and 256 kept u32 bins and four
 * words of state) are allocated on first use and freed by rt_destroy. params == NULL:
 * rt_display_default_params. plane_device: RT_DISPLAY_PLANE's float4 plane of width*height pixels,
 * row-major, in device memory of the context's device, 16-byte aligned; the caller orders its
 * producers before rt_stream(ctx).
 * RT_E_INVALID, with the exposure state and the display plane left as they were: a rank context
 * (world_size > 1); an unknown source, operator or encode value, or auto_exposure above 1;
 * RT_DISPLAY_ACCUMULATION with Params.accumulate != 1 or with no frame since the last reset
 * (rt_denoise's two conditions); RT_DISPLAY_DENOISED before any denoise call; RT_DISPLAY_PLANE with a
 * pointer that is NULL, not device memory of the context's device or not 16-byte aligned; a non-NULL
 * pointer with another source; auto_exposure == 0 with exposure not finite or <= 0; auto_exposure == 1
 * with key, min_exposure or max_exposure not finite or <= 0, min_exposure > max_exposure, adaptation
 * outside (0, 1] or low_permille + high_permille >= 1000; RT_TONE_REINHARD with white not finite or <= 0.
 * rt_read_display: synchronous; the packed RGBA8 plane (width*height u32) of the last rt_display; the
 *   pointer may be NULL. RT_E_INVALID before any rt_display.
 * rt_copy_display_to_device: rt_copy_denoised_to_device for the display plane, with the same arguments
 *   and errors; RT_E_INVALID before any rt_display. Asynchronous.
 * rt_display_state: synchronous; any pointer may be NULL. *exposure: the adapted exposure E (0.0f when
 *   there is none: before the first auto-exposure call and after rt_display_reset); histogram[256] and
 *   *metered: the bins and the metered pixel count (total) of the last auto-exposure call, zeros before
 *   the first.
 * rt_display_reset: drops the adapted exposure (the next auto-exposure call starts from "state none");
 *   RT_OK when there is none. */
#define RT_DISPLAY_ACCUMULATION 0u  /* c = accumulation / D, exactly rt_denoise's c0 */
#define RT_DISPLAY_DENOISED     1u  /* the f32 result of the last rt_denoise / rt_denoise_temporal */
#define RT_DISPLAY_PLANE        2u  /* a caller's float4 plane of width*height pixels in device memory */
#define RT_TONE_LINEAR   0u
#define RT_TONE_REINHARD 1u         /* extended Reinhard with a white point */
#define RT_TONE_ACES     2u         /* Narkowicz's rational fit */
#define RT_ENCODE_NONE 0u           /* the frame's truncating pack (the reference's look) */
#define RT_ENCODE_SRGB 1u           /* inverse of the texture decode table, by search */

typedef struct rt_display_params {
    uint32_t source, tone_operator, encode, auto_exposure;
    float exposure;        /* used as E when auto_exposure == 0 */
    float key;             /* auto: the luminance the metered average is mapped to */
    float min_exposure, max_exposure;
    float adaptation;      /* auto: in (0, 1]; the share of the way to the target taken per call */
    float white;           /* RT_TONE_REINHARD: the input that maps to 1 */
    uint32_t low_permille, high_permille; /* auto: darkest / brightest share of metered pixels ignored */
} rt_display_params;

#if defined(__cplusplus)
static_assert(sizeof(rt_display_params) == 48, "rt_display_params is 48 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_display_params) == 48, "rt_display_params is 48 bytes");
#endif

/* {ACCUMULATION, REINHARD, SRGB, 1,  1.0f, 0.18f, 1/64.f, 64.0f, 1.0f, 4.0f, 100, 50} */
RT_API int rt_display_default_params(rt_display_params* out);
RT_API int rt_display(rt_ctx* ctx, const rt_display_params* params /* NULL: defaults */,
                      const void* plane_device /* RT_DISPLAY_PLANE only, else must be NULL */);
RT_API int rt_read_display(rt_ctx* ctx, uint32_t* rgba8_out);
RT_API int rt_copy_display_to_device(rt_ctx* ctx, void* dst_device, uint32_t bytes_per_row);
RT_API int rt_display_state(rt_ctx* ctx, float* exposure, uint32_t* histogram /* 256 */, uint64_t* metered);
RT_API int rt_display_reset(rt_ctx* ctx);

/* Readback (new: the reference only blits output_data to the swapchain,
 * src/renderer.rs:254-283). Synchronous; whole framebuffer, row-major
 * width*height. Pixels of tiles owned by another rank are left as they were
 * (zero unless written). */
RT_API int rt_read_output(rt_ctx* ctx, uint32_t* rgba8_out);
RT_API int rt_read_accumulation(rt_ctx* ctx, float* rgba_f32_out);

/* Display readback (Renderer::update_texture + calculate_bytes_per_row,
 * src/renderer.rs:254-295): the packed RGBA8 output (byte order R, G, B, A:
 * the Rgba8Unorm texel the reference copies into its display texture) written
 * row by row into `dst`, each row `bytes_per_row` bytes apart (>= 4*width; the
 * reference's wgpu copy needs a multiple of 256, which is what forces its
 * window width to a multiple of 64 pixels, src/main.rs:51-53 -- any pitch
 * works here). Padding bytes are left untouched. Synchronous. */
RT_API int rt_read_output_pitched(rt_ctx* ctx, uint8_t* dst, uint32_t bytes_per_row);

/* Renderer::update_texture on the device (new, ABI 11): the copy_buffer_to_texture of
 * src/renderer.rs:254-283 -- the packed RGBA8 output copied row by row into device
 * memory at `dst_device` (a display texture's staging buffer on the context's device),
 * rows `bytes_per_row` bytes apart (>= 4*width; padding untouched). Stream-ordered
 * after the frames submitted so far (queued frames are launched first), asynchronous:
 * the display observation point of a render loop, with no PCIe transfer and no host
 * wait, as in the reference (which never reads the frame back to the host).
 * RT_E_INVALID (ABI 12) when `dst_device` is not device memory of the context's device,
 * or on a rank context (world_size > 1), whose output holds only its own tiles. */
RT_API int rt_copy_output_to_device(rt_ctx* ctx, void* dst_device, uint32_t bytes_per_row);

/* calculate_bytes_per_row (src/renderer.rs:285-295): 4*width rounded up to
 * `alignment` (a power of two; the reference uses wgpu's 256). 0 on bad input. */
RT_API uint32_t rt_bytes_per_row(uint32_t width, uint32_t alignment);

/* Counted ray segments (every trace_ray call: primary + bounce, a path that
 * escapes to the environment stops counting), summed over all dispatches
 * since creation or the last rt_reset_ray_count. Synchronous. */
RT_API int rt_ray_count(rt_ctx* ctx, uint64_t* out);
RT_API int rt_reset_ray_count(rt_ctx* ctx);

/* Brute-force mode (BASELINE.json config 5, "brute-force LDS-tiled intersect
 * stress"): with enable = 1 later launches run the reference's own sweeps --
 * every sphere (check_spheres, compute_shader.wgsl:355-404), every object's and
 * sub-object's box and the triangles of those hit (check_triangles, :422-517) --
 * with no acceleration structure: a wavefront over the live paths, each
 * workgroup streaming the sub-object records through LDS in tiles and testing
 * them with broadcast reads. enable = 2 (ABI 11): the same sweeps with the
 * records streamed through the scalar cache by each wave (no LDS tile; a scene
 * without triangles has none to stream and runs mode 1's kernel: rt_last_launch_passes
 * says which ran). Same results, bit for bit, as the accelerated default (0); other
 * values are RT_E_INVALID. The scene's spheres, materials and objects must fit in LDS.
 * rt_streamed_bytes: the tile-streaming term of SURVEY §8d for those launches --
 * 32 B x the swept sub-objects per started 256 rays of each bounce level, its fixed
 * convention -- since creation or the last rt_reset_ray_count. rt_streamed_bytes_l2
 * (ABI 12): the sub-object bytes the sweeps actually read from L2 (per LDS tile and
 * workgroup in mode 1, per wave in mode 2). Synchronous. */
RT_API int rt_set_brute_force(rt_ctx* ctx, int enable);
RT_API int rt_streamed_bytes(rt_ctx* ctx, uint64_t* out);
RT_API int rt_streamed_bytes_l2(rt_ctx* ctx, uint64_t* out);

/* Distance pruning of the triangle walk (new; ABI 8, modes since ABI 9). The
 * reference sweeps every object -> sub-object -> triangle
 * (compute_shader.wgsl:422-517); the accelerator replaces the sweep by a walk that
 * culls boxes the ray misses, which is exact by construction.
 * mode 1 (the default): certified pruning -- once a triangle is hit at t, a triangle
 * of a leaf entered beyond t is also skipped (not loaded) when the leaf box, inflated
 * by a derived bound on the f32 error of the reference's triangle test for that
 * triangle (its own normal and two coefficients, the leaf's certificate, tri_cone.h;
 * ABI 10), is entered beyond t; exact by construction. Walks of an
 * LDS-resident accelerator use box culling in this mode. 0: box culling only. 2: the relative slack of
 * ABI 8 (skip boxes entered beyond t * (1 + 1/64) + 2^-10 (|o| + extent) / |d|):
 * faster on scenes without coherent normals, NOT exact -- rays nearly in a
 * triangle's plane near their origin can get another triangle than the sweep's
 * (tests/test_tri_accel_cpu.py builds such rays). Walks of the octant-ordered
 * layouts visit near boxes first in every mode. This call is the only way to select
 * mode 2 (the library reads no environment). Synchronous. */
RT_API int rt_set_triangle_pruning(rt_ctx* ctx, int mode);

/* Exact variants of the launch schedule and of the acceleration structures (new, ABI 12;
 * they were environment variables read at rt_create up to ABI 11), for A/B measurements:
 * every setting renders the same bits as the default. Takes effect from the next launch,
 * at any point of a context's life: frames queued before the call are launched under the
 * setting they were queued with. The key "tile_schedule" is rt_set_tile_schedule (it discards
 * the recorded costs and orders too).
 * Keys and values (default first):
 *   "scene_in_lds" 1|0, "lds_mode" 2|1|0 (highest LDS staging mode), "block_threads"
 *   0|256|512|1024 (0: by occupancy), "waves_per_cu" 0..32 (0: 16), "trav_threshold" 0..63
 *   (0: by scene), "drain_threshold" 0..63 (32), "drain_min_steps" (64), "leaf_batch" 0..8
 *   (0: by scene), "queue_stripes" 1..64 (32), "tile_schedule" 1|0, "frame_parallel" 1|0,
 *   "batch_overlap" 1|0, "batch_schedule" 0|1, "unit_tile_major" 1|0, "frame_par_instance" 1|0
 *   (0: frame-parallel batches run the generic instance of the path kernel), "batch_memory_mb"
 *   (an eighth of device memory), "sphere_bvh" 1|0, "sphere_leaf" 0..64 (0: default),
 *   "sphere_octants" 1|0, "sphere_box_order" 1|0, "tri_bvh" 1|0 (0: the reference's sweep),
 *   "tri_octants" 1|0, "tri_qnodes" 1|0, "coop_leaves" 1|0, "stage_subs" 1|0,
 *   "primary_pass" -1|0|1 (-1: by scene), "primary_threads" 256|64|128|512|1024,
 *   "primary_waves" 8|0, "primary_tile_major" 1|0;
 *   ray queries: "query_chunk" 65536 (1..2^24: rays per staged chunk of rt_trace_rays, rt_occluded and rt_radiance,
 *   points of rt_gather and rt_ambient, probes of rt_probe_sh),
 *   "query_lds_mode" -1|0|1|2 (-1: mode 0 below 262144 rays, else the dispatch's placement;
 *   0..2: the highest LDS staging mode of the query, occlusion and radiance kernels, falling back as a dispatch does),
 *   "gather_chunk" 16384 (1..2^20: points per launch of rt_gather, rt_gather_device, rt_ambient and
 *   rt_ambient_device, 1 KB of partials each),
 *   "nearest_walk" 1|0|2 (1: rt_nearest walks the accelerators, 0: its sweep instance tests every candidate,
 *   2: the walk without the greedy descent that precedes it),
 *   "probe_chunk" 1048576 (1..2^26: paths per launch of rt_probe_sh and rt_probe_sh_device, 16 B of scratch each;
 *   a launch covers whole probes, max(1, probe_chunk / samples) of them);
 *   features and denoiser: "feature_band" 524288 (64..2^24: pixels per traced band of rt_compute_features),
 *   "denoise_lds" 1|0 (1: the filter passes with step 1 and 2 stage tile + halo in LDS, 0: direct loads).
 * RT_E_INVALID for an unknown key or a value out of range. */
RT_API int rt_set_tuning(rt_ctx* ctx, const char* key, int32_t value);

/* Tile claim order (new; the reference dispatches a plain grid,
 * src/renderer.rs:238-249). 0 = tile index order. 1 = cost-ordered (the
 * default): every launch records the rays each of its tiles took, and the
 * first workgroup of a launch to run out of tiles sorts the previous launch's
 * costs (most rays first) into the claim order of the next launch, while the
 * rest of the grid drains its last paths. Launches then end on cheap tiles
 * rather than on long paths. Active for launches in which every wave takes
 * at least 4 tiles on average (else the order cannot matter and the sort
 * would lengthen a short launch). Pixels are independent, so the image is
 * bit-identical under any order. Setting a schedule discards recorded costs
 * and orders (the next two launches run in index order). Asynchronous. */
RT_API int rt_set_tile_schedule(rt_ctx* ctx, uint32_t schedule);
/* The claim order the next launch uses (order[q] = local tile claimed at
 * queue position q; the identity when none is sorted yet) and the rays per
 * tile recorded by the last launch (zero once a later launch sorted them;
 * a frame-parallel batch records the rays of its first frame only).
 * Either pointer may be NULL; each holds the rank's owned tile count
 * (rt_owned_pixel_count / 64). Synchronous. */
RT_API int rt_tile_schedule_state(rt_ctx* ctx, uint32_t* order, uint32_t* costs);

/* Current accumulation counter k (the value the next rt_compute_frame uses). */
RT_API int rt_accumulation_index(const rt_ctx* ctx, uint32_t* out);

/* Timing of path-tracing launches, enabled by rt_set_timing(ctx, 1) before them:
 * each timed launch's span on the device clock, from the start of its first
 * workgroup to the end of its last (s_memrealtime, the same interval rocprofv3's
 * kernel trace reports; overlapped batches' spans overlap). rt_last_dispatch_ms:
 * the last one (milliseconds). Synchronous. */
RT_API int rt_set_timing(rt_ctx* ctx, int enable);
RT_API int rt_last_dispatch_ms(rt_ctx* ctx, float* out_ms);
/* Sum of the timed launch spans since the last rt_reset_timing, and how many
 * launches were timed (read back in bulk on this call, so timing a long run adds
 * no host sync per frame). */
RT_API int rt_dispatch_time_total(rt_ctx* ctx, double* total_ms, uint64_t* n_timed);
/* The same for the resolve pass of timed frame-parallel batches
 * (rt_resolve_frames_kernel: each pixel's lights added to its accumulation in
 * frame order, the last frame's RGBA8 packed), which the path kernel's span above
 * does not include. n_timed counts the batches that had one. */
RT_API int rt_resolve_time_total(rt_ctx* ctx, double* total_ms, uint64_t* n_timed);
RT_API int rt_reset_timing(rt_ctx* ctx);

/* Multi-GPU gather support. The pixels owned by this context's
 * rank, in tile order, are packed into / unpacked from a contiguous device
 * buffer so one RCCL collective moves them. Sizes are in pixels. */
RT_API int rt_owned_pixel_count(const rt_ctx* ctx, uint32_t rank, uint32_t world_size, uint64_t* out);
/* Pack this rank's accumulation (float4 per pixel) into device memory `dst`
 * (rt_owned_pixel_count * 16 bytes). Stream-ordered on the context's stream. */
RT_API int rt_pack_owned_accumulation(rt_ctx* ctx, void* dst_device);
/* Unpack a block packed by `src_rank` of `world_size` into this context's
 * accumulation buffer and re-pack the RGBA8 output for those pixels with
 * the given accumulation divisor (k*c, src/compute_shader.wgsl:166). */
RT_API int rt_unpack_accumulation(rt_ctx* ctx, const void* src_device, uint32_t src_rank, uint32_t world_size,
                           uint32_t divisor);
/* The same for the packed RGBA8 output (one u32 per pixel, rt_owned_pixel_count
 * * 4 bytes), copied as is: the gather of a non-accumulating render
 * (Params.accumulate == 0 never writes the accumulation, compute_shader.wgsl:171-178). */
RT_API int rt_pack_owned_output(rt_ctx* ctx, void* dst_device);
RT_API int rt_unpack_output(rt_ctx* ctx, const void* src_device, uint32_t src_rank, uint32_t world_size);
/* One launch for a whole gather: `src_device` holds world_size consecutive
 * blocks of `stride_px` pixels (>= rank 0's rt_owned_pixel_count, the largest),
 * block r packed by rank r; every block except skip_rank's (the destination's
 * own tiles, already in place; pass world_size or more to unpack all) is
 * unpacked as rt_unpack_accumulation / rt_unpack_output would. */
RT_API int rt_unpack_accumulation_ranks(rt_ctx* ctx, const void* src_device, uint64_t stride_px,
                                        uint32_t world_size, uint32_t skip_rank, uint32_t divisor);
RT_API int rt_unpack_output_ranks(rt_ctx* ctx, const void* src_device, uint64_t stride_px, uint32_t world_size,
                                  uint32_t skip_rank);

/* Launch geometry of the last rt_dispatch (diagnostics): workgroup size in
 * threads, workgroups launched, dynamic LDS bytes per workgroup, and the LDS
 * staging mode (0: scene in global memory, 1: spheres/materials/objects/sphere
 * BVH staged in LDS, 2: also the triangle accelerator). */
RT_API int rt_launch_config(rt_ctx* ctx, uint32_t* threads, uint32_t* blocks, uint32_t* lds_bytes,
                            uint32_t* scene_in_lds);

/* The kernels the last rt_dispatch ran (diagnostics, ABI 7), a mask of RT_PASS_*:
 * the path kernel, the coherent primary-ray pre-pass, the batch resolve pass, or the
 * brute-force sweep kernel instead of the path kernel (with RT_PASS_BRUTE_STREAM, ABI 12:
 * its scalar-cache variant, rt_set_brute_force mode 2). Bit 32 (RT_PASS_TREELET, an ABI-12
 * treelet wavefront measured 2.9x slower than the path kernel on C5 and removed) is not set.
 * RT_PASS_PATH_FRAME_PAR (with RT_PASS_PATH): the path kernel ran as its frame-parallel
 * instance -- a frame-parallel batch with bounces >= 1, unless the tuning key
 * "frame_par_instance" is 0 -- and not as the generic instance that serves every launch. */
#define RT_PASS_PATH 1u
#define RT_PASS_PRIMARY 2u
#define RT_PASS_RESOLVE 4u
#define RT_PASS_BRUTE 8u
#define RT_PASS_BRUTE_STREAM 16u
#define RT_PASS_PATH_FRAME_PAR 64u
RT_API int rt_last_launch_passes(rt_ctx* ctx, uint32_t* passes);

/* Diagnostic counters (filled only by builds compiled with -DRT_DIAG or
 * -DRT_DIAG_TAIL, zeros otherwise): out[0..n) receives up to 8 u64 counters
 * (tools/diag_split.py, tools/tail_probe.py), then, for n > 8, per-wave
 * (start, end) real-time stamps of the last launch (-DRT_DIAG_TAIL). */
RT_API int rt_debug_counters(rt_ctx* ctx, uint64_t* out, uint32_t n);

/* Diagnostics (ABI 10): re-derives every leaf certificate of the certified triangle walk
 * (tri_cone.h) on the host from the device's current leaf records,
 * sub-objects and triangles, and compares them with the records the device built.
 * *mismatches = differing records, *valid = records that carry a certificate, *total =
 * leaf records (all 0 when the last launch read no certificates). */
RT_API int rt_debug_check_leaf_certificates(rt_ctx* ctx, uint32_t* mismatches, uint32_t* valid, uint32_t* total);

/* Device self-check of the kernel's fast exact-arithmetic helpers against the
 * IEEE operations they replace, over every f32 input (current device):
 * which 0 = sqrt on {+-0} U [2^-96, inf], 1..4 = x / 2pi, x / pi, x / 255,
 * x / 10; 5: the Box-Muller log, 6: its cos, on every value random01 returns.
 * *mismatches = number of differing results (0 = bit-exact),
 * *first_bad = smallest differing input's bit pattern (0xffffffff if none). */
RT_API int rt_math_selftest(uint32_t which, uint64_t* mismatches, uint32_t* first_bad);

/* The context's HIP stream (hipStream_t), for callers that want to order
 * their own device work (e.g. an RCCL collective) after a frame. */
RT_API void* rt_stream(rt_ctx* ctx);

/* The 256-entry sRGB -> linear table the kernel decodes Rgba8UnormSrgb
 * texels with (IEC 61966-2-1, rounded to f32). For tests. */
RT_API int rt_srgb_table(float out[256]);

/* ---- several GPUs in one process (SURVEY §5, §8b threading row, §8e) -----
 *
 * The reference renders on one adapter (src/main.rs:636-665). A group is N
 * contexts in this process -- rank r on devices[r], world N: 8x8 tile t is
 * rendered by rank t % N, with global pixel indices for the RNG seeds, so the
 * assembled frame is bit-identical to one GPU's -- each driven by its own host
 * thread, plus one RCCL communicator per device (ncclCommInitAll; librccl is
 * loaded on the first rt_create_multi). Rendering needs no communication;
 * rt_gather_frame assembles the frame on a root device over xGMI.
 *
 * `info` describes the whole frame and scene exactly as for rt_create (rank 0,
 * world_size 0 or 1; its `device` is ignored). Host arrays passed to group calls
 * are copied by every device before the call returns. Calls on one group are not
 * thread-safe. rt_group_compute_frame is asynchronous (each device's thread
 * queues or launches its share); a failure there is returned by the next
 * synchronous group call. rt_group_context gives rank r's context for the
 * single-context entry points -- only while the group is idle (after
 * rt_group_synchronize or a synchronous group call).
 * Group errors: rt_group_last_error(g) (rt_last_error(NULL) for rt_create_multi). */
typedef struct rt_group rt_group;

RT_API int rt_create_multi(const rt_create_info* info, const int32_t* devices, uint32_t n_devices, rt_group** out);
/* rt_create_multi with flags (new, ABI 11). RT_GROUP_COPY_TRANSPORT: no RCCL
 * communicators; rt_gather_frame moves each rank's packed block to the root with a
 * stream-ordered device-to-device copy (hipMemcpyPeerAsync on the sender's stream,
 * after the root's previous unpack; the root's unpack waits for every copy), and a
 * device may be listed more than once -- several ranks of one group on one GPU, which
 * runs the group's N-rank logic (one host thread and context per rank, tile ownership,
 * the root's N receive slots) on a one-GPU machine, or a group where RCCL is absent.
 * The assembled frame is the same bits either way. flags 0 == rt_create_multi. */
#define RT_GROUP_COPY_TRANSPORT 1u
RT_API int rt_create_multi_ex(const rt_create_info* info, const int32_t* devices, uint32_t n_devices, uint32_t flags,
                              rt_group** out);
RT_API void rt_destroy_multi(rt_group* g);
RT_API const char* rt_group_last_error(const rt_group* g);
RT_API uint32_t rt_group_size(const rt_group* g);
RT_API rt_ctx* rt_group_context(rt_group* g, uint32_t rank);

/* Renderer::compute_frame (src/renderer.rs:201-252) on every device's share. */
RT_API int rt_group_compute_frame(rt_group* g, uint32_t bounces);
RT_API int rt_group_set_frame_batch(rt_group* g, uint32_t max_frames);
RT_API int rt_group_flush(rt_group* g);
RT_API int rt_group_synchronize(rt_group* g);
RT_API int rt_group_update_params(rt_group* g, const rt_params* params);
RT_API int rt_group_reset_accumulation(rt_group* g, const rt_params* params);
RT_API int rt_group_update_camera(rt_group* g, const rt_ray_camera* camera);
RT_API int rt_group_update_camera_matrices(rt_group* g, const float inverse_projection[16],
                                           const float inverse_view[16]);
RT_API int rt_group_update_ray_directions(rt_group* g, const rt_ray* rays, uint32_t count);
RT_API int rt_group_update_spheres(rt_group* g, const rt_scene_sphere* spheres, uint32_t count);
RT_API int rt_group_update_triangles(rt_group* g, const rt_scene_triangle* triangles, uint32_t count);
RT_API int rt_group_update_object_info(rt_group* g, const rt_object_info* objects, uint32_t count);
RT_API int rt_group_update_sub_object_info(rt_group* g, const rt_sub_object_info* sub_objects, uint32_t count);
RT_API int rt_group_update_materials(rt_group* g, const rt_scene_material* materials, uint32_t count);
RT_API int rt_group_upload_textures(rt_group* g, const uint8_t* rgba8, uint32_t width, uint32_t height,
                                    uint32_t layers);
RT_API int rt_group_upload_env_map(rt_group* g, const uint8_t* rgba8, uint32_t width, uint32_t height);
/* Counted rays summed over the devices (rt_ray_count). Synchronous. */
RT_API int rt_group_ray_count(rt_group* g, uint64_t* out);
RT_API int rt_group_reset_ray_count(rt_group* g);

/* Gather payloads. */
#define RT_GATHER_IMAGE 0         /* the packed RGBA8 output, 4 B/px: the frame the reference displays */
#define RT_GATHER_ACCUMULATION 1  /* the RGBA32F accumulation, 16 B/px (+ the output rebuilt from it) */
/* Assembles the frame on device `root`: every device packs its tiles
 * (rt_pack_owned_output / rt_pack_owned_accumulation) on its stream, one grouped
 * ncclSend / ncclRecv moves every block (the root's own too) into the root's
 * receive buffer over xGMI, and the root unpacks them all in one launch
 * (rt_unpack_*_ranks; the accumulation payload re-packs the RGBA8 output with the
 * last frame's divisor k*c, compute_shader.wgsl:166). Everything is stream-ordered
 * after the frames submitted so far: the call returns without waiting for the
 * device. Afterwards the root's output (and, for RT_GATHER_ACCUMULATION, its
 * accumulation) equals a one-GPU render's; the other devices keep accumulating
 * their own tiles. */
RT_API int rt_gather_frame(rt_group* g, uint32_t root, uint32_t payload);
/* rt_read_output / rt_read_accumulation of device `root`'s context. Synchronous. */
RT_API int rt_group_read_output(rt_group* g, uint32_t root, uint32_t* rgba8_out);
RT_API int rt_group_read_accumulation(rt_group* g, uint32_t root, float* rgba_f32_out);

/* ---- scene build and edit: src/triangle_object.rs -----
 *
 * Host-side restatement of SceneObject (STL file -> placed triangles -> 7-triangle
 * sub-objects) in f32 with glam's operation order, plus the device-side
 * rebuild that Renderer::update_scene (src/renderer.rs:153-199) runs after an
 * edit. Vertices are 9 floats per triangle (a, b, c), in triangle order.
 * Calls without a context report errors through rt_last_error(NULL). */

/* The edit state of one object (SceneObject::rotation / scale /
 * transformation, src/triangle_object.rs:39-52): rotation in degrees about
 * x, y, z (applied as Rz * Ry * Rx, :253-269). 32 bytes. */
typedef struct rt_object_transform {
    float rotation[3];
    float scale;
    float transformation[3];
    uint32_t _padding;
} rt_object_transform;

/* stl_io::read_stl (src/triangle_object.rs:69): binary or ASCII STL bytes.
 * rt_stl_triangle_count gives the facet count; rt_stl_read writes 9 floats per
 * facet (normals are ignored, as in the reference). */
RT_API int rt_stl_triangle_count(const uint8_t* data, size_t size, uint32_t* count);
RT_API int rt_stl_read(const uint8_t* data, size_t size, float* vertices, uint32_t capacity);

/* SceneObject::new (src/triangle_object.rs:55-127): rotate, normalise to unit
 * diagonal, scale, drop onto the y = 0 surface, translate to `coordinates`.
 * Outputs: the normalised points the edit path starts from (9 floats per
 * triangle), the triangles (SceneTriangle::new), the ObjectInfo (bounds,
 * material; sub-object fields 0) and the initial edit state (scale 1,
 * rotation 0, transformation = coordinates + surface drop). */
RT_API int rt_scene_object_new(const float* stl_vertices, uint32_t triangle_count, float scale,
                               const float coordinates[3], const float rotation[3], uint32_t material_index,
                               float* normalized_points, rt_scene_triangle* triangles, rt_object_info* info,
                               rt_object_transform* state);

/* SceneObject::create_sub_objects (:160-197): chunks of 7 triangles with their
 * AABBs; `sub_objects` has room for ceil(triangle_count / 7). Sets the
 * object's first_sub_object_index / sub_object_count. */
RT_API int rt_scene_object_create_sub_objects(const rt_scene_triangle* triangles, uint32_t triangle_count,
                                              uint32_t first_sub_object_index, uint32_t first_triangle_index,
                                              rt_object_info* info, rt_sub_object_info* sub_objects);

/* SceneObject::update_triangles + update_sub_objects (:129-150, :199-220) on
 * the host: triangles and bounds from the normalised points and `state`.
 * `sub_objects` holds info->sub_object_count records (bounds rewritten). */
RT_API int rt_scene_object_update(const float* normalized_points, uint32_t triangle_count,
                                  const rt_object_transform* state, rt_object_info* info,
                                  rt_scene_triangle* triangles, rt_sub_object_info* sub_objects);

/* Device-side edit path. rt_set_object_models uploads every object's normalised
 * points (9 floats per triangle, in the triangle buffer's order; the objects
 * and sub-objects last set on the context say which triangles belong to which
 * object). rt_update_objects then runs update_triangles + update_sub_objects
 * for objects [0, count) on the device -- triangles, sub-object bounds,
 * object bounds -- and refits the triangle accelerator there, stream-ordered
 * before the next frame: no host round trip. Asynchronous. */
RT_API int rt_set_object_models(rt_ctx* ctx, const float* normalized_points, uint32_t triangle_count);
RT_API int rt_update_objects(rt_ctx* ctx, const rt_object_transform* transforms, uint32_t count);

/* ---- motion records for the temporal denoiser (ABI 12, additive: motion records) ----
 *
 * rt_denoise_temporal reprojects every pixel as if its surface stood still, so a piece the user
 * drags is rejected by the position test and shows a fresh 1-spp estimate on every edit.
 * rt_denoise_temporal_motion takes, per object and per sphere, how that primitive moved since the
 * previous call, reprojects each surface point through its own primitive's motion and validates
 * history against the primitive's identity (the ID plane of the feature buffers).
 *
 * A record says where the surface point that is NOW at X was at the previous call: A X, A = (L | t)
 * a row-major 3x4. flags 0 is a static primitive (m and normal_scale are ignored); RT_MOTION_MOVED
 * uses them; RT_MOTION_DROP gives the primitive's pixels no history (it appeared, teleported or
 * changed material) and wins over MOVED. The records are an input to the contract, like
 * world_to_pixel, not part of it.
 *
 * rt_motion_from_transforms (no context; errors through rt_last_error(NULL)): the records of
 * `count` objects from their edit states at the previous and at the current call, for the pose
 * update_triangles applies, world = Rz Ry Rx(rotation) p scale + transformation with the f32
 * rotation matrix of rt_scene_object_update: L = (s_prev/s_cur) R_prev R_cur^T, t = T_prev - L T_cur,
 * normal_scale = s_cur/s_prev, computed in double and rounded once to f32. A byte-identical pair
 * gives flags 0. RT_E_INVALID: a NULL argument with count > 0, a scale not finite or <= 0.
 *
 * rt_denoise_temporal_motion: rt_denoise_temporal (same slots, generation rule, observation-point
 * behaviour, errors and "changes nothing a render observes") under the motion contract below. The
 * tables are copied before the call returns into a context-owned buffer that grows as needed and is
 * freed by rt_destroy; a table may be NULL with count 0 (everything static). Indices are rt_hit.index:
 * object i of the object buffer, sphere i as uploaded; a primitive beyond its table is static.
 * Further RT_E_INVALID: a NULL table with count > 0, unknown flag bits, a non-finite m or
 * normal_scale in a MOVED record. A failing call leaves the history as it was.
 * STATE. Each slot gains an I plane (uint2, 8 B per pixel), allocated at the first motion call. A
 * slot written by this entry point has ids, one written by rt_denoise_temporal has none (that call's
 * kernel and memory traffic are as before). rt_read_temporal, rt_read_denoised,
 * rt_copy_denoised_to_device and rt_temporal_reset serve both entry points.
 *
 * THE MOTION STAGE (rt_denoise_temporal_motion; tests/temporal_motion_ref.py restates it from here).
 *
 * This is the temporal contract above, word for word, with the changes below. Everything is f32, one
 * IEEE operation per written operation, in the written order, with no contraction.
 *
 * 2m. Record lookup.
 *   id_p comes from the ID plane.
 *   The record R is objects[id.y] if id.x == 2 && id.y < object_count.
 *   R is spheres[id.y] if id.x == 1 && id.y < sphere_count.
 *   Otherwise there is no record. Misses never have one.
 *   X_p is as in step 2.
 *   If R has DROP, the pixel has no history.
 *   If R has MOVED, for i = 0..2:
 *     Y_i = ((m[4i]*X.x + m[4i+1]*X.y) + m[4i+2]*X.z) + m[4i+3];
 *     g_i = ((m[4i]*n.x + m[4i+1]*n.y) + m[4i+2]*n.z) * normal_scale.
 *   Otherwise Y = X_p and g = n_p, chosen by selection. The pixel does no arithmetic.
 *
 * 3m. Projection. Step 3 projects Y instead of X_p.
 *
 * 4m. Tap tests.
 *   The tap tests are those of step 4, with g in the normal test and e = Y - X_q in the position test.
 *   f = X_p - o and r2 are unchanged. The tolerance scales with the current distance.
 *   On a hit, and only when the previous slot has an I plane, one further test applies: both words of
 *   I_q equal id_p.
 *
 * 7m. Store. Store as step 7: X = (X_p, hit_p) and Nn = (n_p, n_out). In addition I = id_p.
 *
 * Steps 1, 5, 6 and 8 are unchanged.
 * End of the motion contract. */
#define RT_MOTION_MOVED 1u /* use m and normal_scale */
#define RT_MOTION_DROP 2u  /* this primitive takes no history (appeared, teleported, re-materialed) */
typedef struct rt_motion {
    float m[12];           /* row-major 3x4 A: where the surface point now at X was at the previous call */
    float normal_scale;    /* n' = (L n) * normal_scale, L the 3x3 part of A */
    uint32_t flags;        /* 0: static. Other bits than MOVED and DROP: RT_E_INVALID */
    uint32_t _reserved[2]; /* 0 */
} rt_motion;

#if defined(__cplusplus)
static_assert(sizeof(rt_motion) == 64, "rt_motion is 64 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rt_motion) == 64, "rt_motion is 64 bytes");
#endif

RT_API int rt_motion_from_transforms(const rt_object_transform* prev, const rt_object_transform* cur, uint32_t count,
                                     rt_motion* out);
RT_API int rt_denoise_temporal_motion(rt_ctx* ctx, const rt_temporal_params* params,
                                      const rt_denoise_params* denoise_params /* NULL: defaults */,
                                      const rt_motion* objects, uint32_t object_count, const rt_motion* spheres,
                                      uint32_t sphere_count);

/* Readback of the scene geometry the kernel sees (after host or device
 * updates). Triangles come back as full 112-byte records. Synchronous. */
RT_API int rt_read_triangles(rt_ctx* ctx, rt_scene_triangle* out, uint32_t count);
RT_API int rt_read_object_info(rt_ctx* ctx, rt_object_info* out, uint32_t count);
RT_API int rt_read_sub_object_info(rt_ctx* ctx, rt_sub_object_info* out, uint32_t count);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RT_ABI_H */
