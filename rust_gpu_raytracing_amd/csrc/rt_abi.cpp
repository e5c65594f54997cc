// rt_abi.cpp — host implementation of include/rt_abi.h.
//
// Replaces the wgpu side of the reference's per-frame path:
//   DataBuffers (src/buffers.rs:140-596)  -> hipMalloc'd device buffers, updated
//                                            through a pinned staging buffer with
//                                            hipMemcpyAsync on the context stream
//   Renderer::compute_frame (src/renderer.rs:201-252)
//                                         -> Params shadow + hipLaunchKernelGGL
// Stream order gives the same visibility guarantees as wgpu's queue order.
//
// This file: the context's life (rt_create, rt_destroy), the uploads and updates, the read-backs,
// the device edit path, rt_set_tuning and the small setters, timing, counters and the debug calls
// of include/rt_abi.h, and the helpers of rt_ctx.h that the other host files call. It launches
// scene_edit.hip's edit and refit kernels and pathtrace.hip's math self-test. The frame launches
// are in rt_frames.cpp, the queries in rt_queries.cpp, features, denoiser and display transform in
// rt_post.cpp.
#include <algorithm>
#include <cmath>
#include <new>

#include "rt_ctx.h"
#include "rt_launch.h"


static_assert(sizeof(rt_params) == 48, "Params is 48 bytes (src/buffers.rs:9-22)");
static_assert(sizeof(rt_ray_camera) == 16, "RayCamera is 16 bytes");
static_assert(sizeof(rt_ray) == 16, "Ray is 16 bytes");
static_assert(sizeof(rt_scene_sphere) == 32, "SceneSphere is 32 bytes");
static_assert(sizeof(rt_scene_triangle) == 112, "SceneTriangle is 112 bytes");
static_assert(sizeof(rt_scene_material) == 32, "SceneMaterial is 32 bytes");
static_assert(sizeof(rt_object_info) == 48, "ObjectInfo is 48 bytes");
static_assert(sizeof(rt_sub_object_info) == 32, "SubObjectInfo is 32 bytes");
static_assert(sizeof(rt_query_ray) == 32, "rt_query_ray is two 16-B loads");
static_assert(sizeof(rt_hit) == 64, "rt_hit is four 16-B stores");
static_assert(sizeof(rt_denoise_params) == 16, "rt_denoise_params is 16 bytes");
static_assert(sizeof(rt_temporal_params) == 80, "rt_temporal_params is 80 bytes");
static_assert(sizeof(rt_motion) == 64 && offsetof(rt_motion, normal_scale) == 48, "rt_motion is four 16-B rows");
static_assert(sizeof(rt_display_params) == 48, "rt_display_params is 48 bytes");
static_assert(sizeof(rt_occlusion_ray) == sizeof(rt_query_ray), "rt_occlusion_ray is an rt_query_ray with t_max for _pad1");
static_assert(sizeof(rt_radiance_ray) == sizeof(rt_query_ray), "rt_radiance_ray is an rt_query_ray with the stream for _pad0");
static_assert(offsetof(rt_radiance_ray, stream) == 12 && offsetof(rt_radiance_ray, direction) == 16,
              "rt_radiance_ray: {origin, stream}, {direction, pad} as two 16-B loads");
static_assert(sizeof(rt_gather_point) == sizeof(rt_radiance_ray), "rt_gather_point has the layout of rt_radiance_ray");
static_assert(offsetof(rt_gather_point, stream) == 12 && offsetof(rt_gather_point, normal) == 16,
              "rt_gather_point: {position, stream}, {normal, pad} as two 16-B loads");
static_assert(sizeof(rt_ambient_point) == sizeof(rt_gather_point), "rt_ambient_point is an rt_gather_point with t_max for _pad1");
static_assert(offsetof(rt_ambient_point, stream) == 12 && offsetof(rt_ambient_point, normal) == 16 &&
                  offsetof(rt_ambient_point, t_max) == 28,
              "rt_ambient_point: {position, stream}, {normal, t_max} as two 16-B loads");
static_assert(sizeof(rt_probe) == 16 && offsetof(rt_probe, stream) == 12, "rt_probe: {position, stream} as one 16-B load");
static_assert(sizeof(rt_scene_material) == sizeof(RtMaterial), "material record");
static_assert(sizeof(rt_object_info) == sizeof(RtObject), "object record");
static_assert(sizeof(rt_sub_object_info) == sizeof(RtSubObject), "sub-object record");

namespace {

// d_counter: [0] the ray counter, [1, 1 + kDiagCounters) the diagnostic
// counters of RT_DIAG / RT_DIAG_TAIL builds (KernelArgs::diag), then the
// per-wave (queue dry, end) records of RT_DIAG_TAIL builds: room for 65,536 waves.
constexpr size_t kDiagCounters = kDiagHeaderWords;
constexpr size_t kDiagWaveRecords = 2 * 65536;
constexpr size_t kCounterWords = 1 + kDiagCounters + kDiagWaveRecords;
constexpr uint32_t kClockSlots = 4096;
constexpr uint32_t kClockWords = 4;  // per timed launch: path kernel {~start, end}, resolve kernel {~start, end}

}  // namespace

// The last error of a call without a context (rt_create, the scene builders).
thread_local std::string g_create_error;
void rt_set_global_error(const std::string& msg) { g_create_error = msg; }

namespace rth {

// Orders the primary stream after everything issued on the auxiliary stream
// (overlapped batches): every call other than rt_compute_frame runs this first.
hipError_t join_aux(rt_ctx* ctx) {
    if (!ctx->aux_outstanding) return hipSuccess;
    ctx->aux_outstanding = false;
    return hipStreamWaitEvent(ctx->stream, ctx->ev_aux_done, 0);
}

int fail(rt_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

int hip_fail(rt_ctx* ctx, const char* what, hipError_t e) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    return fail(ctx, RT_E_HIP, m);
}

// RT_OK when every pointer is device memory of the context's device at its alignment (or NULL
// where that is allowed); else RT_E_INVALID with a message naming `entry` and the argument.
int check_device_ptrs(rt_ctx* ctx, const char* entry, std::initializer_list<DevicePtr> ptrs) {
    auto bad = [&](const DevicePtr& a, const std::string& why) {
        return fail(ctx, RT_E_INVALID, std::string(entry) + ": " + a.name + " " + why);
    };
    for (const DevicePtr& a : ptrs) {
        if (!a.p) {
            if (a.may_be_null) continue;
            return bad(a, "is NULL");
        }
        hipPointerAttribute_t attr{};
        const hipError_t ea = hipPointerGetAttributes(&attr, a.p);
        if (ea != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != ctx->device) {
            (void)hipGetLastError();
            return bad(a, "must be device memory of the context's device");
        }
        if ((uintptr_t)a.p & (a.alignment - 1u))
            return bad(a, "must be " + std::to_string(a.alignment) + "-byte aligned");
    }
    return RT_OK;
}

uint32_t owned_tile_count(uint32_t n_tiles, uint32_t rank, uint32_t world) {
    if (rank >= n_tiles) return 0;
    return (n_tiles - rank + world - 1) / world;
}

// Returns a pinned host region of at least `bytes`, waiting for any copy
// still reading the previous contents.
int staging(rt_ctx* ctx, size_t bytes, void** out) {
    if (ctx->staging_busy) {
        RT_HIP(ctx, hipEventSynchronize(ctx->staging_done));
        ctx->staging_busy = false;
    }
    if (bytes > ctx->pinned_cap) {
        if (ctx->pinned) RT_HIP(ctx, hipHostFree(ctx->pinned));
        ctx->pinned = nullptr;
        ctx->pinned_cap = 0;
        size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes;
        RT_HIP(ctx, hipHostMalloc(&ctx->pinned, cap, hipHostMallocDefault));
        ctx->pinned_cap = cap;
    }
    *out = ctx->pinned;
    return RT_OK;
}

int staged_copy(rt_ctx* ctx, void* dst, size_t bytes) {
    if (bytes == 0) return RT_OK;
    RT_HIP(ctx, hipMemcpyAsync(dst, ctx->pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipEventRecord(ctx->staging_done, ctx->stream));
    ctx->primary_dirty = true;  // an overlapped batch issued later must follow this copy
    ctx->staging_busy = true;
    return RT_OK;
}

int upload_raw(rt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return RT_OK;
    void* p;
    int rc = staging(ctx, bytes, &p);
    if (rc) return rc;
    std::memcpy(p, src, bytes);
    return staged_copy(ctx, dst, bytes);
}

// Rebuild the kernel's sphere slots (brute-force set + BVH) for the first
// `count` spheres and upload them, stream-ordered before the next launch.
int refresh_sphere_slots(rt_ctx* ctx, uint32_t count, bool sphere_only) {
    if (!ctx->slots_dirty && ctx->slots_count == count && ctx->slots_sphere_only == sphere_only) return RT_OK;
    SphereSlots sl;
    build_sphere_slots(ctx->h_sph.data(), count, ctx->use_bvh, &sl, ctx->sphere_leaf_max);
    std::vector<uint32_t> mat(count);
    for (uint32_t i = 0; i < count; i++) mat[i] = ctx->h_sph[i].material_index;
    std::vector<SphereBvhNode> oct;  // 8 direction-ordered copies; layout 0 alone is a complete walk too
    // boxes stored as (near, far) corners per octant when that is exact (rt_bvh_slab.h);
    // only the sphere-only kernels read them that way, so only for scenes without objects
    const bool box_order = ctx->sphere_box_order && sphere_only && box_layout_orderable(sl.nodes);
    order_bvh_by_octant(sl.nodes, &oct, box_order);
    int rc;
    if ((rc = upload_raw(ctx, ctx->d_slot_sph, sl.slot_sph.data(), sl.slot_sph.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_slot_orig, sl.slot_orig.data(), sl.slot_orig.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_sph_mat, mat.data(), mat.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_bvh, oct.data(), oct.size() * sizeof(SphereBvhNode))))
        return rc;
    ctx->n_always = sl.n_always;
    ctx->n_slots = (uint32_t)sl.slot_orig.size();
    ctx->n_nodes = (uint32_t)sl.nodes.size();
    ctx->sphere_boxes_ordered = box_order;
    ctx->sphere_extent = sl.extent;
    ctx->sphere_rmin = sl.r_min;
    ctx->sphere_rmax = sl.r_max;
    ctx->slots_dirty = false;
    ctx->near_radius_dirty = true;  // rt_nearest's table of |radius| holds the spheres the slots were built for
    ctx->slots_count = count;
    ctx->slots_sphere_only = sphere_only;
    return RT_OK;
}

// After device-side edits (rt_update_objects) the host copies of the object and
// sub-object records are stale; read them back before anything host-side uses
// their bounds.
int sync_host_geometry(rt_ctx* ctx) {
    if (!ctx->geom_on_device) return RT_OK;
    if (!ctx->h_obj.empty())
        RT_HIP(ctx, hipMemcpyAsync(ctx->h_obj.data(), ctx->d_obj, ctx->h_obj.size() * 48, hipMemcpyDeviceToHost,
                                   ctx->stream));
    if (!ctx->h_sub.empty())
        RT_HIP(ctx, hipMemcpyAsync(ctx->h_sub.data(), ctx->d_sub, ctx->h_sub.size() * 32, hipMemcpyDeviceToHost,
                                   ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->geom_on_device = false;
    return RT_OK;
}

// Rebuild the triangle accelerator for the first `object_count` objects when
// objects or sub-objects changed (the boxes it culls with are theirs).
int refresh_tri_accel(rt_ctx* ctx, uint32_t object_count) {
    if (!ctx->use_tri_bvh || object_count == 0) return RT_OK;
    if (!ctx->tri_dirty && ctx->tri_count_built == object_count) return RT_OK;
    int rc0 = sync_host_geometry(ctx);
    if (rc0) return rc0;
    int rc;
    TriangleAccel acc;
    build_triangle_accel(ctx->h_obj.data(), object_count, ctx->h_sub.data(), (uint32_t)ctx->h_sub.size(), &acc);
    const size_t nb = acc.nodes.size() * sizeof(SphereBvhNode), pb = acc.prims.size() * sizeof(SubObjectPrim);
    if ((rc = grow_buffer(ctx, "triangle accelerator nodes", &ctx->d_tri_bvh, &ctx->tri_bvh_cap, nb)) ||
        (rc = grow_buffer(ctx, "triangle accelerator leaves", &ctx->d_tri_prims, &ctx->tri_prims_cap, pb)) ||
        (rc = upload_raw(ctx, ctx->d_tri_bvh, acc.nodes.data(), nb)) ||
        (rc = upload_raw(ctx, ctx->d_tri_prims, acc.prims.data(), pb)))
        return rc;
    ctx->qnodes_dirty = true;
    ctx->cones_dirty = true;
    ctx->ltris_dirty = true;
    ctx->tri_nodes = (uint32_t)acc.nodes.size();
    ctx->tri_prim_count = (uint32_t)acc.prims.size();
    ctx->tri_octants_built = false;
    if (ctx->use_tri_octants && acc.nodes.size() > 1 && acc.nodes.size() * 8 < (size_t)kTriWalkEnd) {
        std::vector<SphereBvhNode> oct;
        std::vector<uint32_t> src;
        order_bvh_by_octant(acc.nodes, &oct, false, &src);
        std::vector<uint32_t> skip(oct.size());
        for (size_t i = 0; i < oct.size(); i++) skip[i] = oct[i].skip;
        const size_t b8 = oct.size() * 4;
        if ((rc = grow_buffer(ctx, "octant layout sources", &ctx->d_tri_src8, &ctx->tri_src8_cap, b8)) ||
            (rc = grow_buffer(ctx, "octant layout links", &ctx->d_tri_skip8, &ctx->tri_skip8_cap, b8)) ||
            (rc = grow_buffer(ctx, "octant layout nodes", &ctx->d_tri_bvh8, &ctx->tri_bvh8_cap, oct.size() * sizeof(SphereBvhNode))) ||
            (rc = upload_raw(ctx, ctx->d_tri_src8, src.data(), b8)) ||
            (rc = upload_raw(ctx, ctx->d_tri_skip8, skip.data(), b8)))
            return rc;
        ctx->tri_octants_built = true;
    }
    // depth levels for the device refit (preorder: a node precedes its children)
    std::vector<uint32_t> depth(acc.nodes.size(), 0);
    uint32_t max_depth = 0;
    for (size_t i = 0; i < acc.nodes.size(); i++) {
        max_depth = std::max(max_depth, depth[i]);
        if (acc.nodes[i].leaf == kSphereBvhInternal) {
            depth[i + 1] = depth[i] + 1;
            depth[acc.nodes[i + 1].skip] = depth[i] + 1;
        }
    }
    std::vector<uint32_t> off(max_depth + 2, 0), order(acc.nodes.size());
    for (uint32_t d : depth) off[max_depth - d + 1]++;  // deepest level first
    for (size_t l = 1; l < off.size(); l++) off[l] += off[l - 1];
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    for (size_t i = 0; i < acc.nodes.size(); i++) order[fill[max_depth - depth[i]]++] = (uint32_t)i;
    if ((rc = grow_buffer(ctx, "refit order", &ctx->d_tri_order, &ctx->tri_order_cap, order.size() * 4)) ||
        (rc = grow_buffer(ctx, "refit levels", &ctx->d_tri_level_off, &ctx->tri_level_cap, off.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_tri_order, order.data(), order.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_tri_level_off, off.data(), off.size() * 4)) ||
        (rc = upload_raw(ctx, ctx->d_tri_extent, &acc.extent, 4)))
        return rc;
    ctx->tri_levels = max_depth + 1;
    ctx->tri_dirty = false;
    ctx->tri_count_built = object_count;
    return RT_OK;
}

}  // namespace rth

namespace {

void srgb_table(float out[256]) {
    // IEC 61966-2-1 decode of an 8-bit Rgba8UnormSrgb channel, rounded to f32.
    for (int i = 0; i < 256; i++) {
        const double c = (double)i / 255.0;
        const double l = c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4);
        out[i] = (float)l;
    }
}

int upload_spheres(rt_ctx* ctx, const rt_scene_sphere* s, uint32_t n) {
    if (n == 0) return RT_OK;
    std::copy(s, s + n, ctx->h_sph.begin());
    ctx->slots_dirty = true;  // slots + BVH are rebuilt at the next dispatch
    ctx->near_radius_dirty = true;  // rt_nearest's table of |radius| is rewritten at the next query
    return RT_OK;
}

int upload_triangles(rt_ctx* ctx, const rt_scene_triangle* t, uint32_t n) {
    if (n == 0) return RT_OK;
    ctx->cones_dirty = true;
    ctx->ltris_dirty = true;
    ctx->near_boxes = kNearBoxesUnknown;
    void* p;
    int rc = staging(ctx, (size_t)n * sizeof(RtTriangleHot), &p);
    if (rc) return rc;
    RtTriangleHot* hot = static_cast<RtTriangleHot*>(p);
    for (uint32_t i = 0; i < n; i++) {
        const rt_scene_triangle& s = t[i];
        hot[i] = pack_triangle(s.a, s.edge_ab, s.edge_ac, s.calc_normal, s.face_normal);
    }
    if ((rc = staged_copy(ctx, ctx->d_tri, (size_t)n * sizeof(RtTriangleHot))) ||
        (rc = staging(ctx, (size_t)n * 32, &p)))
        return rc;
    float4* b = static_cast<float4*>(p);
    for (uint32_t i = 0; i < n; i++) {
        const rt_scene_triangle& s = t[i];
        b[2 * i] = make_float4(s.min_bounds[0], s.min_bounds[1], s.min_bounds[2], 0.f);
        b[2 * i + 1] = make_float4(s.max_bounds[0], s.max_bounds[1], s.max_bounds[2], 0.f);
    }
    return staged_copy(ctx, ctx->d_tri_bounds, (size_t)n * 32);
}

// Index ranges the kernel walks must lie inside the buffers (the reference's
// fixed-size WGSL arrays would clamp; here they are rejected up front).
int validate_ranges(rt_ctx* ctx) {
    for (size_t i = 0; i < ctx->h_obj.size(); i++) {
        const rt_object_info& o = ctx->h_obj[i];
        if ((uint64_t)o.first_sub_object_index + o.sub_object_count > ctx->cap_sub)
            return fail(ctx, RT_E_INVALID, "object " + std::to_string(i) + " sub-object range exceeds sub_object_count");
    }
    for (size_t i = 0; i < ctx->h_sub.size(); i++) {
        const rt_sub_object_info& s = ctx->h_sub[i];
        if (s.triangle_count != 0 && (uint64_t)s.first_triangle_index + s.triangle_count > ctx->cap_tri)
            return fail(ctx, RT_E_INVALID, "sub-object " + std::to_string(i) + " triangle range exceeds triangle_count");
    }
    return RT_OK;
}

int check_params(rt_ctx* ctx, const rt_params* p) {
    if (!p) return fail(ctx, RT_E_INVALID, "params is NULL");
    if (p->screen_width != ctx->width)
        return fail(ctx, RT_E_INVALID, "params.screen_width must equal the framebuffer width");
    if (p->sphere_count > ctx->cap_sph) return fail(ctx, RT_E_INVALID, "params.sphere_count exceeds sphere buffer");
    if (p->object_count > ctx->cap_obj) return fail(ctx, RT_E_INVALID, "params.object_count exceeds object buffer");
    return RT_OK;
}

int collect_timing(rt_ctx* ctx) {
    if (ctx->clock_pending.empty()) return RT_OK;
    RT_HIP(ctx, join_aux(ctx));
    std::vector<unsigned long long> c(kClockWords * (size_t)kClockSlots);
    RT_HIP(ctx, hipMemcpyAsync(c.data(), ctx->d_clock, c.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t slot : ctx->clock_pending) {
        const unsigned long long* w = c.data() + kClockWords * (size_t)slot;
        const unsigned long long t0 = ~w[0], t1 = w[1];
        if (w[0] != 0 && t1 >= t0) {  // else no workgroup ran
            const float ms = (float)((double)(t1 - t0) / ctx->wall_khz);
            ctx->total_ms += ms;
            ctx->n_timed += 1;
            ctx->last_ms = ms;
        }
        const unsigned long long r0 = ~w[2], r1 = w[3];
        if (w[2] != 0 && r1 >= r0) {  // the batch's resolve pass
            ctx->resolve_total_ms += (double)(r1 - r0) / ctx->wall_khz;
            ctx->n_resolve_timed += 1;
        }
    }
    ctx->clock_pending.clear();
    // the slots start the next launches at zero (the kernels atomicMax into them): cleared
    // here, off the launch path, instead of by a memset ahead of every timed launch
    RT_HIP(ctx, hipMemsetAsync(ctx->d_clock, 0, c.size() * 8, ctx->stream));
    ctx->primary_dirty = true;  // an auxiliary-stream batch waits for it
    return RT_OK;
}

}  // namespace

namespace rth {

// The auxiliary stream follows the primary stream: what S runs next waits for everything issued
// on the primary stream so far (nothing to do when S is the primary stream).
hipError_t follow_primary(rt_ctx* ctx, hipStream_t S) {
    if (S == ctx->stream) return hipSuccess;
    const hipError_t e = hipEventRecord(ctx->ev_primary, ctx->stream);
    return e != hipSuccess ? e : hipStreamWaitEvent(S, ctx->ev_primary, 0);
}

// ka.launch_clock: the timing slot of a launch on stream S, null unless timing is on
// (rt_set_timing, which also allocates the ring ahead of the launches).
int claim_clock_slot(rt_ctx* ctx, hipStream_t S, KernelArgs& ka) {
    ka.launch_clock = nullptr;
    if (!ctx->timing) return RT_OK;
    int rc;
    if (ctx->clock_pending.size() >= kClockSlots && (rc = collect_timing(ctx))) return rc;
    if (!ctx->d_clock) {
        if ((rc = dev_alloc(ctx, &ctx->d_clock, kClockWords * (size_t)kClockSlots))) return rc;
        RT_HIP(ctx, follow_primary(ctx, S));  // the zeroed slots must be in place before an aux launch
    }
    const uint32_t slot = ctx->clock_next;
    ctx->clock_next = (ctx->clock_next + 1) % kClockSlots;
    ka.launch_clock = ctx->d_clock + kClockWords * (size_t)slot;  // zero: dev_alloc / collect_timing
    ctx->clock_pending.push_back(slot);
    return RT_OK;
}

}  // namespace rth

int rt_abi_version(void) { return RT_ABI_VERSION; }

#ifndef RT_BUILD_HASH
#define RT_BUILD_HASH "unknown"
#endif
const char* rt_build_hash(void) { return RT_BUILD_HASH; }

const char* rt_last_error(const rt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rt_srgb_table(float out[256]) {
    if (!out) return RT_E_INVALID;
    srgb_table(out);
    return RT_OK;
}

int rt_create(const rt_create_info* info, rt_ctx** out_ctx) {
    g_create_error.clear();
    if (!info || !out_ctx) return fail(nullptr, RT_E_INVALID, "rt_create: NULL argument");
    *out_ctx = nullptr;
    if (info->width == 0 || info->height == 0) return fail(nullptr, RT_E_INVALID, "width and height must be > 0");
    if (info->world_size == 0 || info->rank >= info->world_size)
        return fail(nullptr, RT_E_INVALID, "rank must be < world_size (world_size >= 1)");
    const uint64_t n_pixels = (uint64_t)info->width * info->height;
    if (n_pixels > 0xffffffffull) return fail(nullptr, RT_E_INVALID, "pixel index must fit in u32 (:148)");
    if (!info->camera_rays) return fail(nullptr, RT_E_INVALID, "camera_rays is NULL");
    if ((info->material_count && !info->materials) || (info->sphere_count && !info->spheres) ||
        (info->triangle_count && !info->triangles) || (info->object_count && !info->objects) ||
        (info->sub_object_count && !info->sub_objects))
        return fail(nullptr, RT_E_INVALID, "NULL scene array with a non-zero count");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        return fail(nullptr, RT_E_NODEVICE, "no HIP device available");
    if (info->device < 0 || info->device >= n_dev) return fail(nullptr, RT_E_NODEVICE, "device ordinal out of range");

    rt_ctx* ctx = new (std::nothrow) rt_ctx();
    if (!ctx) return fail(nullptr, RT_E_NOMEM, "out of host memory");
    auto bail = [&](int rc) {
        g_create_error = ctx->err;
        rt_destroy(ctx);
        return rc;
    };
    ctx->device = info->device;
    ctx->width = info->width;
    ctx->height = info->height;
    ctx->n_pixels = n_pixels;
    ctx->rank = info->rank;
    ctx->world = info->world_size;
    ctx->tiles_x = (info->width + 7) / 8;
    ctx->tiles_y = (info->height + 7) / 8;
    ctx->owned_tiles = owned_tile_count(ctx->tiles_x * ctx->tiles_y, ctx->rank, ctx->world);
    ctx->camera = info->camera;
    ctx->cap_mat = info->material_count;
    ctx->cap_sph = info->sphere_count;
    ctx->cap_tri = info->triangle_count;
    ctx->cap_obj = info->object_count;
    ctx->cap_sub = info->sub_object_count;
    ctx->n_mat_dev = info->material_count ? info->material_count : 1;
    ctx->n_tri_dev = info->triangle_count ? info->triangle_count : 1;
    ctx->n_sub_dev = info->sub_object_count ? info->sub_object_count : 1;
    ctx->h_obj.assign(info->objects, info->objects + info->object_count);
    ctx->h_sph.resize(info->sphere_count);
    ctx->h_sub.assign(info->sub_objects, info->sub_objects + info->sub_object_count);

    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return bail(hip_fail(ctx, "hipSetDevice", e));
    {
        int n_cu = 0;
        e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device);
        if (e != hipSuccess) return bail(hip_fail(ctx, "hipDeviceGetAttribute", e));
        ctx->n_cu = n_cu;
        // the batch buffers' share of device memory: an eighth of the device
        size_t free_b = 0, total_b = 0;
        e = hipMemGetInfo(&free_b, &total_b);
        if (e != hipSuccess) return bail(hip_fail(ctx, "hipMemGetInfo", e));
        ctx->batch_budget = total_b / 8;
    }
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return bail(hip_fail(ctx, "hipStreamCreate", e));
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) == hipSuccess && khz > 0)
            ctx->wall_khz = (double)khz;
    }
    e = hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return bail(hip_fail(ctx, "hipStreamCreate (aux)", e));
    for (hipEvent_t* ev : {&ctx->staging_done, &ctx->ev_resolved[0], &ctx->ev_resolved[1], &ctx->ev_aux_done,
                           &ctx->ev_primary}) {
        e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e != hipSuccess) return bail(hip_fail(ctx, "hipEventCreate", e));
    }

    int rc;
    if ((rc = check_params(ctx, &info->params))) return bail(rc);
    if ((rc = validate_ranges(ctx))) return bail(rc);
    ctx->params = info->params;
    ctx->k = 1;  // src/renderer.rs:96

    if ((rc = dev_alloc(ctx, &ctx->d_rays, n_pixels)) || (rc = dev_alloc(ctx, &ctx->d_accum, n_pixels)) ||
        (rc = dev_alloc(ctx, &ctx->d_out, n_pixels)) || (rc = dev_alloc(ctx, &ctx->d_counter, kCounterWords)) ||
        (rc = dev_alloc(ctx, &ctx->d_queue, 4 * kQueueStripesMax * kQueueStride)) ||  // 2 streams x 2 halves
        (rc = dev_alloc(ctx, &ctx->d_slot_sph, 4 * (size_t)info->sphere_count + 4)) ||  // padded groups
        (rc = dev_alloc(ctx, &ctx->d_slot_orig, 4 * (size_t)info->sphere_count + 4)) ||
        (rc = dev_alloc(ctx, &ctx->d_sph_mat, info->sphere_count)) ||
        (rc = dev_alloc(ctx, &ctx->d_bvh, 16 * (size_t)info->sphere_count + 8)) ||  // 8 ordered layouts
        (rc = dev_alloc(ctx, &ctx->d_mat, ctx->n_mat_dev)) || (rc = dev_alloc(ctx, &ctx->d_obj, info->object_count)) ||
        (rc = dev_alloc(ctx, &ctx->d_sub, ctx->n_sub_dev)) || (rc = dev_alloc(ctx, &ctx->d_tri, ctx->n_tri_dev)) ||
        (rc = dev_alloc(ctx, &ctx->d_tri_bounds, 2 * (size_t)ctx->n_tri_dev)) ||
        (rc = dev_alloc(ctx, &ctx->d_tri_extent, 1)) || (rc = dev_alloc(ctx, &ctx->d_stream, 2)) ||
        (rc = dev_alloc(ctx, &ctx->d_srgb, 256)) || (rc = dev_alloc(ctx, &ctx->d_tex, 1)) ||
        (rc = dev_alloc(ctx, &ctx->d_env, 1)))
        return bail(rc);
    ctx->tex_w = ctx->tex_h = ctx->tex_layers = 1;  // a black 1x1 placeholder until textures arrive
    ctx->env_w = ctx->env_h = 1;

    if ((rc = upload_raw(ctx, ctx->d_rays, info->camera_rays, n_pixels * 16)) ||
        (rc = upload_raw(ctx, ctx->d_mat, info->materials, (size_t)info->material_count * 32)) ||
        (rc = upload_spheres(ctx, info->spheres, info->sphere_count)) ||
        (rc = upload_triangles(ctx, info->triangles, info->triangle_count)) ||
        (rc = upload_raw(ctx, ctx->d_obj, info->objects, (size_t)info->object_count * 48)) ||
        (rc = upload_raw(ctx, ctx->d_sub, info->sub_objects, (size_t)info->sub_object_count * 32)))
        return bail(rc);
    float lut[256];
    srgb_table(lut);
    if ((rc = upload_raw(ctx, ctx->d_srgb, lut, sizeof(lut)))) return bail(rc);
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return bail(hip_fail(ctx, "hipStreamSynchronize", e));
    ctx->staging_busy = false;
    *out_ctx = ctx;
    return RT_OK;
}

void rt_destroy(rt_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)flush_frames(ctx);  // queued frames were submitted: they run before teardown
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
    void* bufs[] = {ctx->d_rays, ctx->d_accum, ctx->d_out, ctx->d_counter, ctx->d_queue, ctx->d_slot_sph,
                    ctx->d_slot_orig, ctx->d_bvh, ctx->d_sph_mat, ctx->d_tri_bvh, ctx->d_tri_prims,
                    ctx->d_mat,  ctx->d_obj,   ctx->d_sub, ctx->d_tri,     ctx->d_tex,     ctx->d_env,
                    ctx->d_srgb, ctx->d_tri_extent, ctx->d_tri_order, ctx->d_tri_level_off, ctx->d_model,
                    ctx->d_tri_object, ctx->d_sub_object, ctx->d_object_tris, ctx->d_place, ctx->d_tri_bounds,
                    ctx->d_tile_sched[0], ctx->d_tile_sched[1], ctx->d_frame_light[0], ctx->d_frame_light[1],
                    ctx->d_clock, ctx->d_stream, ctx->d_primary[0], ctx->d_primary[1], ctx->d_tri_qnodes,
                    ctx->d_tri_qgrid, ctx->d_tri_src8, ctx->d_tri_skip8, ctx->d_tri_bvh8, ctx->d_tri_lcert,
                    ctx->d_tri_ltris, ctx->d_brute_paths, ctx->d_brute_queue, ctx->d_brute_counts,
                    ctx->d_query_next, ctx->d_query_buf, ctx->d_radiance_segs, ctx->d_gather_partials, ctx->d_probe_lights, ctx->d_probe_next, ctx->d_lens_cam, ctx->d_near_radius, ctx->d_feat[0], ctx->d_feat[1], ctx->d_feat_scratch,
                    ctx->d_dn[0], ctx->d_dn[1], ctx->d_dn_out, ctx->d_disp_out, ctx->d_disp_meter,
                    ctx->t_slot[0].plane[0], ctx->t_slot[0].plane[1], ctx->t_slot[0].plane[2],
                    ctx->t_slot[1].plane[0], ctx->t_slot[1].plane[1], ctx->t_slot[1].plane[2],
                    ctx->d_feat_ids, ctx->t_slot[0].ids, ctx->t_slot[1].ids, ctx->d_motion};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->query_pinned) (void)hipHostFree(ctx->query_pinned);
    for (hipEvent_t ev : {ctx->staging_done, ctx->ev_resolved[0], ctx->ev_resolved[1], ctx->ev_aux_done,
                          ctx->ev_primary})
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
    delete ctx;
}

int rt_upload_textures(rt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t layers) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (!rgba8 || width == 0 || height == 0 || layers == 0)
        return fail(ctx, RT_E_INVALID, "textures: need non-empty RGBA8 data");
    const size_t texels = (size_t)width * height * layers;
    if (texels != (size_t)ctx->tex_w * ctx->tex_h * ctx->tex_layers || !ctx->d_tex) {
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_tex) RT_HIP(ctx, hipFree(ctx->d_tex));
        ctx->d_tex = nullptr;
        RT_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_tex), texels * 4));
    }
    ctx->tex_w = width;
    ctx->tex_h = height;
    ctx->tex_layers = layers;
    return upload_raw(ctx, ctx->d_tex, rgba8, texels * 4);
}

int rt_upload_env_map(rt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (!rgba8 || width == 0 || height == 0) return fail(ctx, RT_E_INVALID, "env map: need non-empty RGBA8 data");
    const size_t texels = (size_t)width * height;
    if (texels != (size_t)ctx->env_w * ctx->env_h || !ctx->d_env) {
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_env) RT_HIP(ctx, hipFree(ctx->d_env));
        ctx->d_env = nullptr;
        RT_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_env), texels * 4));
    }
    ctx->env_w = width;
    ctx->env_h = height;
    // A map whose rows (columns) are each one colour returns the same texel for
    // any u (v): the kernel then skips that coordinate's atan2 (asin).
    const uint32_t* t = reinterpret_cast<const uint32_t*>(rgba8);
    bool rows = true, cols = true;
    for (size_t y = 0; y < height && rows; y++)
        for (size_t x = 1; x < width; x++)
            if (t[y * width + x] != t[y * width]) {
                rows = false;
                break;
            }
    for (size_t y = 1; y < height && cols; y++)
        for (size_t x = 0; x < width; x++)
            if (t[y * width + x] != t[x]) {
                cols = false;
                break;
            }
    ctx->env_uniform = (rows ? 1u : 0u) | (cols ? 2u : 0u);
    return upload_raw(ctx, ctx->d_env, rgba8, texels * 4);
}

int rt_update_params(rt_ctx* ctx, const rt_params* params) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    int rc = check_params(ctx, params);
    if (rc) return rc;
    ctx->params = *params;
    return RT_OK;
}

int rt_reset_accumulation(rt_ctx* ctx, const rt_params* params) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    int rc = check_params(ctx, params);
    if (rc) return rc;
    RT_HIP(ctx, hipMemsetAsync(ctx->d_accum, 0, ctx->n_pixels * 16, ctx->stream));
    ctx->params = *params;
    ctx->k = params->accumulation_index;
    ++ctx->accum_gen;  // rt_denoise_temporal: a new accumulation generation
    return RT_OK;
}

int rt_update_ray_directions(rt_ctx* ctx, const rt_ray* rays, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !rays) return fail(ctx, RT_E_INVALID, "rays is NULL");
    if (count > ctx->n_pixels) return fail(ctx, RT_E_CAPACITY, "more rays than pixels");
    ctx->gen_rays = false;
    return upload_raw(ctx, ctx->d_rays, rays, (size_t)count * 16);
}

int rt_update_camera_matrices(rt_ctx* ctx, const float inverse_projection[16], const float inverse_view[16]) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (!inverse_projection || !inverse_view) return fail(ctx, RT_E_INVALID, "matrix is NULL");
    std::memcpy(ctx->inv_proj, inverse_projection, sizeof(ctx->inv_proj));
    std::memcpy(ctx->inv_view, inverse_view, sizeof(ctx->inv_view));
    ctx->gen_rays = true;
    return RT_OK;
}

int rt_update_camera(rt_ctx* ctx, const rt_ray_camera* camera) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (!camera) return fail(ctx, RT_E_INVALID, "camera is NULL");
    ctx->camera = *camera;  // passed by value to the next launch
    return RT_OK;
}

int rt_update_spheres(rt_ctx* ctx, const rt_scene_sphere* spheres, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !spheres) return fail(ctx, RT_E_INVALID, "spheres is NULL");
    if (count > ctx->cap_sph) return fail(ctx, RT_E_CAPACITY, "more spheres than the buffer holds");
    return upload_spheres(ctx, spheres, count);
}

int rt_update_triangles(rt_ctx* ctx, const rt_scene_triangle* triangles, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !triangles) return fail(ctx, RT_E_INVALID, "triangles is NULL");
    if (count > ctx->cap_tri) return fail(ctx, RT_E_CAPACITY, "more triangles than the buffer holds");
    return upload_triangles(ctx, triangles, count);
}

int rt_update_object_info(rt_ctx* ctx, const rt_object_info* objects, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !objects) return fail(ctx, RT_E_INVALID, "objects is NULL");
    if (count > ctx->cap_obj) return fail(ctx, RT_E_CAPACITY, "more objects than the buffer holds");
    int rc0 = sync_host_geometry(ctx);
    if (rc0) return rc0;
    std::vector<rt_object_info> saved = ctx->h_obj;
    std::copy(objects, objects + count, ctx->h_obj.begin());
    int rc = validate_ranges(ctx);
    if (rc) {
        ctx->h_obj.swap(saved);
        return rc;
    }
    // the accelerator culls with the object boxes and walks the sub-object
    // ranges; the device edit path's maps follow the ranges. A change of the
    // other fields (material_index) invalidates neither.
    bool boxes = false, ranges = false;
    for (uint32_t i = 0; i < count; i++) {
        const rt_object_info &a = saved[i], &b = objects[i];
        boxes |= std::memcmp(a.min_bounds, b.min_bounds, 12) != 0 || std::memcmp(a.max_bounds, b.max_bounds, 12) != 0;
        ranges |= a.first_sub_object_index != b.first_sub_object_index || a.sub_object_count != b.sub_object_count;
    }
    if (boxes || ranges) ctx->tri_dirty = true;
    if (ranges) ctx->near_boxes = kNearBoxesUnknown;
    if (ranges) ctx->models_valid = false;
    return upload_raw(ctx, ctx->d_obj, objects, (size_t)count * 48);
}

int rt_update_sub_object_info(rt_ctx* ctx, const rt_sub_object_info* sub_objects, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !sub_objects) return fail(ctx, RT_E_INVALID, "sub_objects is NULL");
    if (count > ctx->cap_sub) return fail(ctx, RT_E_CAPACITY, "more sub-objects than the buffer holds");
    int rc0 = sync_host_geometry(ctx);
    if (rc0) return rc0;
    std::vector<rt_sub_object_info> saved = ctx->h_sub;
    std::copy(sub_objects, sub_objects + count, ctx->h_sub.begin());
    int rc = validate_ranges(ctx);
    if (rc) {
        ctx->h_sub.swap(saved);
        return rc;
    }
    for (uint32_t i = 0; i < count; i++)
        if (saved[i].first_triangle_index != sub_objects[i].first_triangle_index ||
            saved[i].triangle_count != sub_objects[i].triangle_count)
            ctx->models_valid = false;  // the device edit path's triangle maps are stale
    ctx->tri_dirty = true;
    ctx->near_boxes = kNearBoxesUnknown;
    return upload_raw(ctx, ctx->d_sub, sub_objects, (size_t)count * 32);
}

int rt_update_materials(rt_ctx* ctx, const rt_scene_material* materials, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !materials) return fail(ctx, RT_E_INVALID, "materials is NULL");
    if (count > ctx->cap_mat) return fail(ctx, RT_E_CAPACITY, "more materials than the buffer holds");
    return upload_raw(ctx, ctx->d_mat, materials, (size_t)count * 32);
}

int rt_read_output(rt_ctx* ctx, uint32_t* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_out, ctx->n_pixels * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_read_output_pitched(rt_ctx* ctx, uint8_t* dst, uint32_t bytes_per_row) {
    RT_ENTER(ctx);
    if (!dst) return fail(ctx, RT_E_INVALID, "dst is NULL");
    if ((uint64_t)bytes_per_row < 4ull * ctx->width) return fail(ctx, RT_E_INVALID, "bytes_per_row < 4 * width");
    RT_HIP(ctx, hipMemcpy2DAsync(dst, bytes_per_row, ctx->d_out, 4ull * ctx->width, 4ull * ctx->width, ctx->height,
                                 hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

uint32_t rt_bytes_per_row(uint32_t width, uint32_t alignment) {
    if (alignment == 0 || (alignment & (alignment - 1)) != 0) return 0;
    const uint64_t v = 4ull * width;
    const uint64_t r = (v + alignment - 1) & ~(uint64_t)(alignment - 1);
    return r > 0xffffffffull ? 0u : (uint32_t)r;
}

// ---- device-side edit path (scene_edit.hip) --------------------------------

int rt_set_object_models(rt_ctx* ctx, const float* points, uint32_t triangle_count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (triangle_count && !points) return fail(ctx, RT_E_INVALID, "normalized_points is NULL");
    if (triangle_count > ctx->cap_tri) return fail(ctx, RT_E_CAPACITY, "more triangles than the buffer holds");
    int rc = sync_host_geometry(ctx);
    if (rc) return rc;
    // triangle -> object and sub-object -> object maps, per-object triangle ranges
    const uint32_t n_obj = (uint32_t)ctx->h_obj.size(), n_sub = (uint32_t)ctx->h_sub.size();
    std::vector<uint32_t> tri_obj(std::max<uint32_t>(triangle_count, 1), 0xffffffffu);
    std::vector<uint32_t> sub_obj(std::max<uint32_t>(n_sub, 1), 0xffffffffu);
    std::vector<uint2> obj_tris(std::max<uint32_t>(n_obj, 1), make_uint2(0, 0));
    for (uint32_t o = 0; o < n_obj; o++) {
        const rt_object_info& ob = ctx->h_obj[o];
        uint32_t first = 0, count = 0;
        for (uint32_t i = 0; i < ob.sub_object_count; i++) {
            const uint32_t si = ob.first_sub_object_index + i;
            const rt_sub_object_info& so = ctx->h_sub[si];
            if (count == 0) first = so.first_triangle_index;
            if (so.triangle_count && so.first_triangle_index != first + count)
                return fail(ctx, RT_E_INVALID, "object " + std::to_string(o) + ": sub-object triangles not contiguous");
            if ((uint64_t)so.first_triangle_index + so.triangle_count > triangle_count)
                return fail(ctx, RT_E_INVALID, "object " + std::to_string(o) + " has triangles without model points");
            sub_obj[si] = o;
            for (uint32_t t = 0; t < so.triangle_count; t++) tri_obj[so.first_triangle_index + t] = o;
            count += so.triangle_count;
        }
        obj_tris[o] = make_uint2(first, count);
    }
    auto alloc = [&](auto** p, size_t count) -> int {
        if (*p) return RT_OK;
        return dev_alloc(ctx, p, count);
    };
    if ((rc = alloc(&ctx->d_model, 9 * (size_t)ctx->n_tri_dev)) || (rc = alloc(&ctx->d_tri_object, ctx->n_tri_dev)) ||
        (rc = alloc(&ctx->d_sub_object, ctx->n_sub_dev)) || (rc = alloc(&ctx->d_object_tris, std::max(ctx->cap_obj, 1u))) ||
        (rc = alloc(&ctx->d_place, std::max(ctx->cap_obj, 1u))) ||
        (rc = upload_raw(ctx, ctx->d_model, points, (size_t)triangle_count * 36)) ||
        (rc = upload_raw(ctx, ctx->d_tri_object, tri_obj.data(), (size_t)triangle_count * 4)) ||
        (rc = upload_raw(ctx, ctx->d_sub_object, sub_obj.data(), (size_t)n_sub * 4)) ||
        (rc = upload_raw(ctx, ctx->d_object_tris, obj_tris.data(), (size_t)n_obj * 8)))
        return rc;
    ctx->model_tris = triangle_count;
    ctx->models_valid = true;
    return RT_OK;
}

int rt_update_objects(rt_ctx* ctx, const rt_object_transform* transforms, uint32_t count) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (count && !transforms) return fail(ctx, RT_E_INVALID, "transforms is NULL");
    if (count > ctx->h_obj.size()) return fail(ctx, RT_E_CAPACITY, "more transforms than objects");
    if (count == 0) return RT_OK;
    if (!ctx->d_model || !ctx->models_valid)
        return fail(ctx, RT_E_INVALID,
                    "object models missing or stale (object / sub-object ranges changed): call rt_set_object_models");
    void* p;
    int rc = staging(ctx, (size_t)count * sizeof(rt_scene::Placement), &p);
    if (rc) return rc;
    rt_scene::Placement* pl = static_cast<rt_scene::Placement*>(p);
    for (uint32_t o = 0; o < count; o++)
        rt_scene::placement(*reinterpret_cast<const rt_scene::ObjectTransform*>(&transforms[o]), pl[o]);
    if ((rc = staged_copy(ctx, ctx->d_place, (size_t)count * sizeof(rt_scene::Placement)))) return rc;
    RT_HIP(ctx, rt_launch_edit(ctx->d_model, ctx->d_tri_object, ctx->d_sub_object, ctx->d_object_tris, ctx->d_place,
                               count, ctx->model_tris, (uint32_t)ctx->h_sub.size(), ctx->d_tri, ctx->d_tri_bounds,
                               ctx->d_sub, ctx->d_obj, ctx->stream));
    ctx->geom_on_device = true;
    // the edit rewrites triangles and boxes on the device (a placement may make them non-finite):
    // rt_nearest looks at them again before it culls by them
    ctx->near_boxes = kNearBoxesUnknown;
    // the accelerator keeps its topology; its boxes (and the margin extent) follow the new bounds
    if (ctx->d_tri_bvh && ctx->tri_nodes && !ctx->tri_dirty) {
        RT_HIP(ctx, rt_launch_refit(ctx->d_tri_bvh, ctx->d_tri_prims, ctx->d_sub, ctx->d_tri_order,
                                    ctx->d_tri_level_off, ctx->tri_levels, ctx->d_tri_extent, ctx->stream));
        ctx->qnodes_dirty = true;
    }
    ctx->cones_dirty = true;  // the triangles changed
    ctx->ltris_dirty = true;
    return RT_OK;
}

int rt_read_triangles(rt_ctx* ctx, rt_scene_triangle* out, uint32_t count) {
    RT_ENTER(ctx);
    if (count && !out) return fail(ctx, RT_E_INVALID, "out is NULL");
    if (count > ctx->cap_tri) return fail(ctx, RT_E_CAPACITY, "more triangles than the buffer holds");
    if (count == 0) return RT_OK;
    std::vector<RtTriangleHot> hot(count);
    std::vector<float4> b(2 * (size_t)count);
    RT_HIP(ctx, hipMemcpyAsync(hot.data(), ctx->d_tri, (size_t)count * sizeof(RtTriangleHot), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(b.data(), ctx->d_tri_bounds, (size_t)count * 32, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    auto put = [](float* dst, const float4& v) {
        dst[0] = v.x;
        dst[1] = v.y;
        dst[2] = v.z;
    };
    for (uint32_t i = 0; i < count; i++) {
        rt_scene_triangle& t = out[i];
        std::memset(&t, 0, sizeof(t));
        unpack_triangle(hot[i], t.a, t.edge_ab, t.edge_ac, t.calc_normal, t.face_normal);
        put(t.min_bounds, b[2 * i]);
        put(t.max_bounds, b[2 * i + 1]);
    }
    return RT_OK;
}

int rt_read_object_info(rt_ctx* ctx, rt_object_info* out, uint32_t count) {
    RT_ENTER(ctx);
    if (count && !out) return fail(ctx, RT_E_INVALID, "out is NULL");
    if (count > ctx->cap_obj) return fail(ctx, RT_E_CAPACITY, "more objects than the buffer holds");
    if (count == 0) return RT_OK;
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_obj, (size_t)count * 48, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_read_sub_object_info(rt_ctx* ctx, rt_sub_object_info* out, uint32_t count) {
    RT_ENTER(ctx);
    if (count && !out) return fail(ctx, RT_E_INVALID, "out is NULL");
    if (count > ctx->cap_sub) return fail(ctx, RT_E_CAPACITY, "more sub-objects than the buffer holds");
    if (count == 0) return RT_OK;
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_sub, (size_t)count * 32, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_read_accumulation(rt_ctx* ctx, float* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_accum, ctx->n_pixels * 16, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_ray_count(rt_ctx* ctx, uint64_t* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    unsigned long long v = 0;
    RT_HIP(ctx, hipMemcpyAsync(&v, ctx->d_counter, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = v;
    return RT_OK;
}

int rt_set_brute_force(rt_ctx* ctx, int enable) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (enable < 0 || enable > 2) return fail(ctx, RT_E_INVALID, "brute-force mode must be 0, 1 or 2");
    ctx->brute = enable;
    return RT_OK;
}

int rt_set_triangle_pruning(rt_ctx* ctx, int mode) {
    RT_ENTER(ctx);
    ++ctx->scene_epoch;  // the feature planes (rt_compute_features) are stale
    if (mode < 0 || mode > 2) return fail(ctx, RT_E_INVALID, "triangle pruning mode must be 0, 1 or 2");
    ctx->tri_prune_mode = mode;
    return RT_OK;
}

int rt_streamed_bytes(rt_ctx* ctx, uint64_t* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    unsigned long long v[2] = {0, 0};
    RT_HIP(ctx, hipMemcpyAsync(v, ctx->d_stream, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = v[0];
    return RT_OK;
}

int rt_streamed_bytes_l2(rt_ctx* ctx, uint64_t* out) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    unsigned long long v[2] = {0, 0};
    RT_HIP(ctx, hipMemcpyAsync(v, ctx->d_stream, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = v[1];
    return RT_OK;
}

// rt_set_tile_schedule and the tuning key "tile_schedule": the claim order, with the recorded costs
// and orders of both streams discarded (after RT_ENTER: the primary stream follows the auxiliary one).
static int set_tile_schedule(rt_ctx* ctx, uint32_t schedule) {
    ctx->tile_schedule = schedule;
    for (int si = 0; si < 2; si++) {
        if (ctx->d_tile_sched[si])
            RT_HIP(ctx, hipMemsetAsync(ctx->d_tile_sched[si], 0, (4 * (size_t)ctx->owned_tiles + 2) * 4, ctx->stream));
        ctx->sched_launches[si] = 0;
    }
    return RT_OK;
}

// Exact variants of the schedule and the acceleration structures, for A/B measurements (the
// product reads no environment): every setting renders the same bits.
int rt_set_tuning(rt_ctx* ctx, const char* key, int32_t value) {
    RT_ENTER(ctx);
    if (!key) return fail(ctx, RT_E_INVALID, "rt_set_tuning: key is NULL");
    const std::string k(key);
    const int32_t v = value;
    auto range = [&](int32_t lo, int32_t hi) {
        return v >= lo && v <= hi ? RT_OK
                                  : fail(ctx, RT_E_INVALID, "rt_set_tuning: " + k + " must be in [" + std::to_string(lo) +
                                                                ", " + std::to_string(hi) + "]");
    };
    auto flag = [&](bool& field) {
        const int rc = range(0, 1);
        if (rc == RT_OK) field = v != 0;
        return rc;
    };
    int rc = RT_OK;
    if (k == "scene_in_lds") {
        if ((rc = range(0, 1)) == RT_OK) ctx->force_global_scene = v == 0;
    } else if (k == "lds_mode") {
        if ((rc = range(0, 2)) == RT_OK) ctx->max_lds_mode = v;
    } else if (k == "block_threads") {
        if (v != 0 && v != 256 && v != 512 && v != 1024)
            return fail(ctx, RT_E_INVALID, "rt_set_tuning: block_threads must be 0, 256, 512 or 1024");
        ctx->force_threads = (uint32_t)v;
    } else if (k == "waves_per_cu") {
        if ((rc = range(0, 32)) == RT_OK) ctx->waves_cap = (uint32_t)v;
    } else if (k == "tri_bvh") {
        if ((rc = flag(ctx->use_tri_bvh)) == RT_OK) ctx->tri_dirty = true;
    } else if (k == "tri_octants") {
        if ((rc = flag(ctx->use_tri_octants)) == RT_OK) ctx->tri_dirty = true;
    } else if (k == "tri_qnodes") {
        rc = flag(ctx->use_qnodes);
    } else if (k == "coop_leaves") {
        rc = flag(ctx->use_coop_leaves);
    } else if (k == "stage_subs") {
        rc = flag(ctx->stage_subs);
    } else if (k == "primary_pass") {
        if ((rc = range(-1, 1)) == RT_OK) ctx->primary_pass = v;
    } else if (k == "primary_threads") {
        if (v != 64 && v != 128 && v != 256 && v != 512 && v != 1024)
            return fail(ctx, RT_E_INVALID, "rt_set_tuning: primary_threads must be 64, 128, 256, 512 or 1024");
        ctx->primary_threads = (uint32_t)v;
    } else if (k == "primary_waves") {
        if (v != 0 && v != 8) return fail(ctx, RT_E_INVALID, "rt_set_tuning: primary_waves must be 0 or 8");
        ctx->primary_min_waves = (uint32_t)v;
    } else if (k == "primary_tile_major") {
        rc = flag(ctx->primary_tile_major);
    } else if (k == "sphere_bvh") {
        if ((rc = flag(ctx->use_bvh)) == RT_OK) ctx->slots_dirty = true;
    } else if (k == "sphere_leaf") {
        if ((rc = range(0, 64)) == RT_OK) {
            ctx->sphere_leaf_max = (uint32_t)v;
            ctx->slots_dirty = true;
        }
    } else if (k == "sphere_octants") {
        rc = flag(ctx->sphere_octants);
    } else if (k == "sphere_box_order") {
        if ((rc = flag(ctx->sphere_box_order)) == RT_OK) ctx->slots_dirty = true;
    } else if (k == "queue_stripes") {
        if ((rc = range(1, (int32_t)kQueueStripesMax)) == RT_OK) ctx->queue_stripes = (uint32_t)v;
    } else if (k == "trav_threshold") {
        if ((rc = range(0, 63)) == RT_OK) ctx->trav_threshold = (uint32_t)v;
    } else if (k == "drain_threshold") {
        if ((rc = range(0, 63)) == RT_OK) ctx->drain_threshold = (uint32_t)v;
    } else if (k == "drain_min_steps") {
        if ((rc = range(0, 1 << 20)) == RT_OK) ctx->drain_min_steps = (uint32_t)v;
    } else if (k == "leaf_batch") {
        if ((rc = range(0, 8)) == RT_OK) ctx->leaf_batch = (uint32_t)v;
    } else if (k == "tile_schedule") {
        if ((rc = range(0, 1)) == RT_OK) rc = set_tile_schedule(ctx, (uint32_t)v);
    } else if (k == "frame_parallel") {
        rc = flag(ctx->frame_parallel);
    } else if (k == "batch_overlap") {
        rc = flag(ctx->batch_overlap);
    } else if (k == "batch_schedule") {
        rc = flag(ctx->batch_schedule);
    } else if (k == "unit_tile_major") {
        rc = flag(ctx->unit_tile_major);
    } else if (k == "frame_par_instance") {
        rc = flag(ctx->frame_par_instance);
    } else if (k == "query_chunk") {
        if ((rc = range(1, (int32_t)kMaxQueryChunk)) == RT_OK) ctx->query_chunk = (uint32_t)v;
    } else if (k == "gather_chunk") {
        if ((rc = range(1, (int32_t)kMaxGatherChunk)) == RT_OK) ctx->gather_chunk = (uint32_t)v;
    } else if (k == "probe_chunk") {
        if ((rc = range(1, (int32_t)kMaxProbeChunk)) == RT_OK) ctx->probe_chunk = (uint32_t)v;
    } else if (k == "nearest_walk") {
        if ((rc = range(0, 2)) == RT_OK) ctx->nearest_walk = v;
    } else if (k == "query_lds_mode") {
        if ((rc = range(-1, 2)) == RT_OK) ctx->query_lds_mode = v;
    } else if (k == "feature_band") {
        if ((rc = range(64, (int32_t)kMaxFeatureBand)) == RT_OK) ctx->feature_band = (uint32_t)v;
    } else if (k == "denoise_lds") {
        rc = flag(ctx->denoise_lds);
    } else if (k == "batch_memory_mb") {
        if ((rc = range(1, 1 << 30)) == RT_OK) ctx->batch_budget = (size_t)v << 20;
    } else {
        return fail(ctx, RT_E_INVALID, "rt_set_tuning: unknown key " + k);
    }
    return rc;
}

int rt_set_tile_schedule(rt_ctx* ctx, uint32_t schedule) {
    RT_ENTER(ctx);
    if (schedule > 1) return fail(ctx, RT_E_INVALID, "tile schedule must be 0 (index order) or 1 (cost-ordered)");
    return set_tile_schedule(ctx, schedule);
}

int rt_tile_schedule_state(rt_ctx* ctx, uint32_t* order, uint32_t* costs) {
    RT_ENTER(ctx);
    // the primary stream's schedule: the one every single-frame launch and every
    // other overlapped batch follows
    const size_t n = ctx->owned_tiles;
    const uint32_t* st = ctx->d_tile_sched[0];
    const uint64_t launches = ctx->sched_launches[0];
    const bool on = ctx->tile_schedule && st;
    const uint32_t par = (uint32_t)(launches & 1u);  // the next launch's parity
    for (size_t i = 0; i < n && order; i++) order[i] = (uint32_t)i;
    if (order && on && launches)
        RT_HIP(ctx, hipMemcpyAsync(order, st + 2 * n + par * n, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (costs) {
        if (on && launches)  // what the last launch recorded
            RT_HIP(ctx, hipMemcpyAsync(costs, st + (par ^ 1u) * n, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        else
            std::memset(costs, 0, n * 4);
    }
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_reset_ray_count(rt_ctx* ctx) {
    RT_ENTER(ctx);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_counter, 0, (1 + kDiagCounters) * sizeof(unsigned long long), ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(ctx->d_stream, 0, 2 * sizeof(unsigned long long), ctx->stream));
    return RT_OK;
}

int rt_accumulation_index(const rt_ctx* ctx, uint32_t* out) {
    if (!ctx || !out) return RT_E_INVALID;
    *out = ctx->k;
    return RT_OK;
}

int rt_set_timing(rt_ctx* ctx, int enable) {
    RT_ENTER(ctx);
    ctx->timing = enable != 0;
    // The launch-clock slots are allocated (and zeroed) here rather than by the first timed
    // launch: callers switch timing on ahead of the region they time (bench.py), which then
    // holds no hipMalloc on its launch path.
    if (ctx->timing && !ctx->d_clock) {
        const int rc = dev_alloc(ctx, &ctx->d_clock, kClockWords * (size_t)kClockSlots);
        if (rc) return rc;
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RT_OK;
}

int rt_last_dispatch_ms(rt_ctx* ctx, float* out_ms) {
    RT_ENTER(ctx);
    if (!out_ms) return fail(ctx, RT_E_INVALID, "out is NULL");
    int rc = collect_timing(ctx);
    if (rc) return rc;
    *out_ms = ctx->last_ms;
    return RT_OK;
}

int rt_dispatch_time_total(rt_ctx* ctx, double* total_ms, uint64_t* n_timed) {
    RT_ENTER(ctx);
    if (!total_ms || !n_timed) return fail(ctx, RT_E_INVALID, "out is NULL");
    int rc = collect_timing(ctx);
    if (rc) return rc;
    *total_ms = ctx->total_ms;
    *n_timed = ctx->n_timed;
    return RT_OK;
}

int rt_resolve_time_total(rt_ctx* ctx, double* total_ms, uint64_t* n_timed) {
    RT_ENTER(ctx);
    if (!total_ms || !n_timed) return fail(ctx, RT_E_INVALID, "out is NULL");
    int rc = collect_timing(ctx);
    if (rc) return rc;
    *total_ms = ctx->resolve_total_ms;
    *n_timed = ctx->n_resolve_timed;
    return RT_OK;
}

int rt_reset_timing(rt_ctx* ctx) {
    RT_ENTER(ctx);
    int rc = collect_timing(ctx);
    if (rc) return rc;
    ctx->total_ms = 0.0;
    ctx->n_timed = 0;
    ctx->resolve_total_ms = 0.0;
    ctx->n_resolve_timed = 0;
    ctx->last_ms = 0.0f;
    return RT_OK;
}

int rt_debug_counters(rt_ctx* ctx, uint64_t* out, uint32_t n) {
    RT_ENTER(ctx);
    if (!out) return fail(ctx, RT_E_INVALID, "out is NULL");
    const size_t m = std::min<size_t>(n, kDiagCounters + kDiagWaveRecords);
    RT_HIP(ctx, hipMemcpyAsync(out, ctx->d_counter + 1, m * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_debug_check_leaf_certificates(rt_ctx* ctx, uint32_t* mismatches, uint32_t* valid, uint32_t* total) {
    RT_ENTER(ctx);
    if (!mismatches || !valid || !total) return fail(ctx, RT_E_INVALID, "NULL output");
    *mismatches = *valid = *total = 0;
    RT_HIP(ctx, join_aux(ctx));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t n = ctx->tri_prim_count;
    if (!ctx->d_tri_lcert || ctx->cones_dirty || n == 0 || ctx->tri_lcert_cap < (size_t)n * sizeof(TriLeafCert))
        return RT_OK;
    std::vector<TriLeafCert> dev(n);
    std::vector<SubObjectPrim> prims(n);
    std::vector<RtSubObject> subs(ctx->n_sub_dev);
    std::vector<RtTriangleHot> tris(ctx->n_tri_dev);
    RT_HIP(ctx, hipMemcpy(dev.data(), ctx->d_tri_lcert, n * sizeof(TriLeafCert), hipMemcpyDeviceToHost));
    RT_HIP(ctx, hipMemcpy(prims.data(), ctx->d_tri_prims, n * sizeof(SubObjectPrim), hipMemcpyDeviceToHost));
    RT_HIP(ctx, hipMemcpy(subs.data(), ctx->d_sub, subs.size() * sizeof(RtSubObject), hipMemcpyDeviceToHost));
    RT_HIP(ctx, hipMemcpy(tris.data(), ctx->d_tri, tris.size() * sizeof(RtTriangleHot), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        const RtSubObject& s = subs[std::min<uint32_t>(prims[i].sub, (uint32_t)subs.size() - 1u)];
        float lo[3], hi[3];
        for (int k = 0; k < 3; k++) {
            lo[k] = std::fmin(s.min_bounds[k], s.max_bounds[k]);
            hi[k] = std::fmax(s.min_bounds[k], s.max_bounds[k]);
        }
        const uint32_t n_tri = (uint32_t)tris.size();
        const uint32_t cnt = (s.triangle_count <= kLeafCertSlots && n_tri != 0u) ? s.triangle_count : 0u;
        float a[kLeafCertSlots][3], ab[kLeafCertSlots][3], ac[kLeafCertSlots][3], cn[kLeafCertSlots][3];
        for (uint32_t j = 0; j < cnt; ++j) {
            float fn[3];
            unpack_triangle(tris[std::min(s.first_triangle_index + j, n_tri - 1u)], a[j], ab[j], ac[j], cn[j], fn);
        }
        const TriLeafCert h = tricone::leafcert_build(cnt, a, ab, ac, cn, lo, hi);
        *mismatches += std::memcmp(&h, &dev[i], sizeof(h)) != 0;
        *valid += dev[i].w[7] != kLeafCertNone;
    }
    *total = n;
    return RT_OK;
}

int rt_launch_config(rt_ctx* ctx, uint32_t* threads, uint32_t* blocks, uint32_t* lds_bytes,
                     uint32_t* scene_in_lds) {
    RT_ENTER(ctx);  // the last launch: queued frames launched first
    if (!threads || !blocks || !lds_bytes || !scene_in_lds) return RT_E_INVALID;
    *threads = ctx->last_threads;
    *blocks = ctx->last_blocks;
    *lds_bytes = ctx->last_lds;
    *scene_in_lds = ctx->last_mode < 0 ? 0u : (uint32_t)ctx->last_mode;
    return RT_OK;
}

int rt_last_launch_passes(rt_ctx* ctx, uint32_t* passes) {
    RT_ENTER(ctx);  // the last launch: queued frames launched first
    if (!passes) return RT_E_INVALID;
    *passes = ctx->last_passes;
    return RT_OK;
}

void* rt_stream(rt_ctx* ctx) {
    if (!ctx) return nullptr;
    // flush_frames may launch and allocate: on the context's device
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    // work the caller orders on this stream follows every frame submitted so far
    if (flush_frames(ctx) != RT_OK || join_aux(ctx) != hipSuccess) return nullptr;
    ctx->primary_dirty = true;
    return (void*)ctx->stream;
}

int rt_math_selftest(uint32_t which, uint64_t* mismatches, uint32_t* first_bad) {
    if (!mismatches || !first_bad || which > 6) return RT_E_INVALID;
    unsigned long long* d_bad = nullptr;
    uint32_t* d_first = nullptr;
    hipError_t e = hipMalloc(&d_bad, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&d_first, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d_bad, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_first, 0xff, sizeof(uint32_t));
    if (e == hipSuccess) e = rt_launch_math_selftest(which, d_bad, d_first, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first_bad, d_first, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (d_bad) (void)hipFree(d_bad);
    if (d_first) (void)hipFree(d_first);
    if (e != hipSuccess) return RT_E_HIP;
    *mismatches = bad;
    return RT_OK;
}
