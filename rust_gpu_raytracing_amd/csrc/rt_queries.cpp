// rt_queries.cpp — the query families of include/rt_abi.h, host and device forms.
//
// rt_trace_rays, rt_pick, rt_occluded, rt_trace_hits, rt_pick_hits, rt_radiance, rt_gather,
// rt_ambient, rt_probe_sh, rt_lens, rt_lens_rays and rt_nearest: one descriptor-driven path
// (QueryFamily, staged_query, device_query) around each family's run. It launches query.hip,
// occlusion.hip, hits.hip, radiance.hip, ambient.hip and nearest.hip.
#include <algorithm>
#include <cmath>

#include "rt_ctx.h"
#include "rt_launch.h"
#include "rt_nearest_math.h"
#include "rt_query_schedule.h"

namespace {

// A query of fewer rays than this launches the mode-0 instance (the scene read from global
// memory) instead of staging the LDS image in every workgroup: measured crossover, DESIGN.md §5.4b.
constexpr uint64_t kQueryStageMinRays = 262144;
// The most samples a probe takes: one probe's scratch is then 256 MiB.
constexpr uint32_t kMaxProbeSamples = 1u << 24;
constexpr size_t kMaxProbeScratchBytes = (size_t)kMaxProbeSamples * 16u;

}  // namespace

// ---- ray queries (query.hip) -------------------------------------------------------------------
//
// A query reads the scene and writes the caller's records, nothing else: the queued frames stay
// queued (nothing changed the scene since they were queued -- every update launches them first --
// so they render the same bits before or after the query), and the accumulation, the output, the
// counters, the timing totals and the tile schedule are not touched. The accelerators are
// prepared exactly as a frame launch prepares them (the same refresh and derivation, whichever
// comes first does the work), on the primary stream after everything the auxiliary stream runs.
int rth::query_enter(rt_ctx* ctx) {
    RT_HIP(ctx, join_aux(ctx));
    if (!ctx->d_query_next) {
        const int rc = dev_alloc(ctx, &ctx->d_query_next, 1);
        if (rc) return rc;
    }
    const rt_params& p = ctx->params;
    int rc = refresh_sphere_slots(ctx, p.sphere_count, p.object_count == 0);
    if (rc) return rc;
    return refresh_tri_accel(ctx, p.object_count);
}

// The scene view of a query of `count` rays: the frame launches' carve, with the placement capped
// by tuning "query_lds_mode", or by default at mode 0 for batches too small to repay staging.
// `kind`: the kernel the view is for -- rt_query_kernel, rt_occlusion_kernel (occlusion.hip) or
// rt_radiance_kernel (radiance.hip), whose `count` is its walks' lower bound, rays x samples, or
// its gather instance (points x samples) or its probe instance (probes x samples), or
// rt_ambient_kernel (ambient.hip; points x samples), or the radiance kernel's lens instance
// (pixels x samples), or rt_hits_kernel (hits.hip), or rt_nearest_kernel (nearest.hip), its walk
// instance or its sweep instance.
enum QueryKind {
    kQueryClosest = 0,
    kQueryAnyHit = 1,
    kQueryRadiance = 2,
    kQueryGather = 3,
    kQueryProbe = 4,
    kQueryAmbient = 5,
    kQueryLens = 6,
    kQueryHits = 7,
    kQueryNearest = 8,
    kQueryNearestSweep = 9
};

static hipError_t nearest_walk_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return rt_nearest_occupancy(mode, tris, false, lds_bytes, blocks_per_cu);
}
static hipError_t nearest_sweep_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return rt_nearest_occupancy(mode, tris, true, lds_bytes, blocks_per_cu);
}

// Per kind: the workgroup size of the instance for a placement, and its resident workgroups per CU.
static const struct {
    uint32_t (*threads)(int mode, bool tris);
    hipError_t (*occupancy)(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu);
} kQueryKernels[10] = {{rt_query_threads, rt_query_occupancy},
                      {rt_occlusion_threads, rt_occlusion_occupancy},
                      {rt_radiance_threads, rt_radiance_occupancy},
                      {rt_radiance_threads, rt_gather_occupancy},
                      {rt_radiance_threads, rt_probe_occupancy},
                      {rt_ambient_threads, rt_ambient_occupancy},
                      {rt_radiance_threads, rt_lens_occupancy},
                      {rt_hits_threads, rt_hits_occupancy},
                      {rt_nearest_threads, nearest_walk_occupancy},
                      {rt_nearest_threads, nearest_sweep_occupancy}};

struct QueryLaunch {
    KernelArgs ka{};
    SceneLaunch sl;
    size_t lds_bytes = 0;
    uint32_t waves_per_block = 0;
    uint64_t resident = 0;  // workgroups of the instance that the device holds at once
};

static int query_scene(rt_ctx* ctx, uint64_t count, int kind, QueryLaunch& q) {
    KernelArgs& ka = q.ka;
    SceneLaunch& sl = q.sl;
    scene_base_args(ctx, ka);
    ka.camera_rays = ctx->d_rays;
    int max_mode = ctx->force_global_scene ? 0 : ctx->max_lds_mode;
    if (ctx->query_lds_mode >= 0)
        max_mode = ctx->query_lds_mode;
    else if (count < kQueryStageMinRays)
        max_mode = 0;
    for (;; --max_mode) {
        // (the carve reads ka.tri_nodes of the single layout: scene_accel_args may have scaled it)
        ka.tri_nodes = ka.tri_accel ? ctx->tri_nodes : 0u;
        ka.tri_bvh = reinterpret_cast<const float4*>(ctx->d_tri_bvh);
        scene_carve(ctx, ka, max_mode, sl);
        const int rc = scene_accel_args(ctx, ka, sl);
        if (rc) return rc;
        const uint32_t threads = kQueryKernels[kind].threads(sl.mode, sl.tris);
        ka.lds_leafbatch_offset = (uint32_t)al16(sl.lds_bytes);
        q.lds_bytes = sl.coop ? ka.lds_leafbatch_offset + (size_t)(threads / 64u) * kLeafBatchWaveBytes : sl.lds_bytes;
        const rt_ctx::QueryOccKey key{sl.mode, kind, sl.tris ? 1u : 0u, (uint32_t)q.lds_bytes};
        if (ctx->q_occ_blocks == 0 || !same_key(ctx->q_occ_key, key)) {
            int n = 0;
            const hipError_t e = kQueryKernels[kind].occupancy(sl.mode, sl.tris, q.lds_bytes, &n);
            if (e != hipSuccess) (void)hipGetLastError();
            ctx->q_occ_key = key;
            ctx->q_occ_blocks = e == hipSuccess ? n : 0;
        }
        if (ctx->q_occ_blocks > 0) break;
        // an image this instance cannot take: the next lower placement (mode 0 fits every scene)
        if (sl.mode == 0) return fail(ctx, RT_E_HIP, "ray query: the kernel does not fit the device");
        max_mode = sl.mode;
    }
    q.waves_per_block = kQueryKernels[kind].threads(sl.mode, sl.tris) / 64u;
    q.resident = (uint64_t)ctx->q_occ_blocks * (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 1);
    return RT_OK;
}

// Traces `count` rays at device pointer `rays` into `hits`, stream-ordered on the primary stream:
// rt_hit records, or with `any_hit` one occlusion byte per rt_occlusion_ray.
int rth::run_query(rt_ctx* ctx, const void* rays, void* hits, uint64_t count, bool any_hit) {
    if (count == 0) return RT_OK;
    QueryLaunch q;
    const int rc = query_scene(ctx, count, any_hit ? kQueryAnyHit : kQueryClosest, q);
    if (rc) return rc;
    // the closest-hit kernel takes every chunk from the counter; an any-hit wave owns its first
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident,
                                                     any_hit ? rtq::kNoChunkCap : 0u, rtq::kWalkChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    const hipError_t e = (any_hit ? rt_launch_occlusion : rt_launch_query)(
        q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, rays, hits, count, ctx->d_query_next, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, any_hit ? "rt_occlusion_kernel launch" : "rt_query_kernel launch", e);
    return RT_OK;
}

// The staging of the host entry points and rt_pick: `n` rays then `n` records, on the device and
// pinned.
static int query_buffers(rt_ctx* ctx, size_t n) {
    if (ctx->query_buf_rays < n) {
        const int rc = grow_buffer(ctx, "query scratch", &ctx->d_query_buf, &ctx->query_buf_bytes, n * (sizeof(rt_query_ray) + sizeof(rt_hit)));
        if (rc) return rc;
        ctx->query_buf_rays = n;
    }
    if (ctx->query_pinned_rays < n) {
        if (ctx->query_pinned) RT_HIP(ctx, hipHostFree(ctx->query_pinned));
        ctx->query_pinned = nullptr;
        ctx->query_pinned_rays = 0;
        RT_HIP(ctx, hipHostMalloc(&ctx->query_pinned, n * (sizeof(rt_query_ray) + sizeof(rt_hit)), hipHostMallocDefault));
        ctx->query_pinned_rays = n;
    }
    return RT_OK;
}

// What the two entry points of a query family differ in from those of the other families; the rest
// of an entry point is staged_query (the host form) or device_query (the device form) around the
// family's run(device in, device out, n, device segment counter or null).
struct QueryFamily {
    const char* host;      // the entry points, as the messages name them
    const char* device;
    const char* in;        // the record arguments, as the messages name them
    const char* out;
    size_t in_bytes;       // per record
    size_t out_bytes;
    uintptr_t out_align;   // of the device form's `out` (its `in` is 16-byte aligned, `segments` 8)
    uint32_t max_samples;  // 0: the family takes no `samples`
    bool segments;         // the family counts ray segments
};
constexpr uint32_t kAnySamples = UINT32_MAX;

// The checks on `samples`, which come first: an entry point refuses them whatever `count` is.
static int check_samples(rt_ctx* ctx, const QueryFamily& f, const char* entry, uint32_t samples) {
    if (f.max_samples == 0) return RT_OK;
    if (samples == 0) return fail(ctx, RT_E_INVALID, std::string(entry) + ": samples is 0");
    if (samples > f.max_samples)
        return fail(ctx, RT_E_INVALID, std::string(entry) + ": samples above " + std::to_string(f.max_samples));
    return RT_OK;
}

// The device form of a family's entry point: `count` records at device pointer `in` answered into
// `out`, stream-ordered on the primary stream; `segments` (device memory too) may be null.
template <class Run>
static int device_query(rt_ctx* ctx, const QueryFamily& f, const void* in, void* out, uint64_t count, uint32_t samples,
                        void* segments, Run run) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_samples(ctx, f, f.device, samples);
    if (rc || count == 0) return rc;
    rc = check_device_ptrs(ctx, f.device,
                           {{in, f.in, 16, false}, {out, f.out, f.out_align, false}, {segments, "segments", 8, true}});
    if (rc || (rc = query_enter(ctx))) return rc;
    return run(in, out, count, static_cast<unsigned long long*>(segments));
}

// The staging of a host form, after its checks: the `count` records of `in_bytes` each at host pointer
// `in` go through the pinned and the device scratch in chunks of "query_chunk"; run answers a
// chunk, and `out_bytes` per record come back to `out`. Both scratch buffers hold the inputs at
// their base and the results at capacity x 32 bytes (where the records of a closest-hit chunk go);
// a call whose results exceed 32 bytes per record (rt_probe_sh: 144) sizes both by that many
// records more. In a family that counts segments the context's segment counter is zeroed first and
// read back after the last chunk, into the pinned bytes after a chunk's results, for `segments`
// (which may be null). A family without input records (in_bytes == 0: the lens families, whose
// range starts at record `first`) uploads nothing, and its run takes the index of the chunk's
// first record where the others take the chunk's device input.
template <class Run>
static int staged_chunks(rt_ctx* ctx, const QueryFamily& f, const void* in, uint64_t first, void* out, uint64_t count,
                         uint64_t* segments, Run run) {
    int rc;
    if (f.segments && !ctx->d_radiance_segs && (rc = dev_alloc(ctx, &ctx->d_radiance_segs, 1))) return rc;
    const size_t in_bytes = f.in_bytes, out_bytes = f.out_bytes;
    const size_t chunk = (size_t)std::min<uint64_t>(count, ctx->query_chunk);
    if ((rc = query_buffers(ctx, chunk * ((out_bytes + 31u) / 32u)))) return rc;
    unsigned char* d_in = static_cast<unsigned char*>(ctx->d_query_buf);
    unsigned char* d_out = d_in + ctx->query_buf_rays * sizeof(rt_query_ray);
    unsigned char* h_in = static_cast<unsigned char*>(ctx->query_pinned);
    unsigned char* h_out = h_in + ctx->query_pinned_rays * sizeof(rt_query_ray);
    unsigned long long* h_segs = reinterpret_cast<unsigned long long*>(h_out + chunk * out_bytes);
    unsigned long long* d_segs = f.segments ? ctx->d_radiance_segs : nullptr;
    if (d_segs) RT_HIP(ctx, hipMemsetAsync(d_segs, 0, sizeof(unsigned long long), ctx->stream));
    for (uint64_t done = 0; done < count;) {
        const size_t n = (size_t)std::min<uint64_t>(chunk, count - done);
        if constexpr (std::is_invocable_v<Run, uint64_t, void*, uint64_t, unsigned long long*>) {
            if ((rc = run(first + done, d_out, n, d_segs))) return rc;
        } else {
            std::memcpy(h_in, static_cast<const unsigned char*>(in) + done * in_bytes, n * in_bytes);
            RT_HIP(ctx, hipMemcpyAsync(d_in, h_in, n * in_bytes, hipMemcpyHostToDevice, ctx->stream));
            if ((rc = run(d_in, d_out, n, d_segs))) return rc;
        }
        RT_HIP(ctx, hipMemcpyAsync(h_out, d_out, n * out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (d_segs && done + n == count)
            RT_HIP(ctx, hipMemcpyAsync(h_segs, d_segs, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(static_cast<unsigned char*>(out) + done * out_bytes, h_out, n * out_bytes);
        done += n;
    }
    if (d_segs && segments) *segments = *h_segs;
    return RT_OK;
}

// The host form of a family's entry point: its checks, then the staging of its records.
template <class Run>
static int staged_query(rt_ctx* ctx, const QueryFamily& f, const void* in, void* out, uint64_t count, uint32_t samples,
                        uint64_t* segments, Run run) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_samples(ctx, f, f.host, samples);
    if (rc) return rc;
    if (count == 0) {
        if (segments) *segments = 0;
        return RT_OK;
    }
    if (!in || !out) return fail(ctx, RT_E_INVALID, std::string(f.host) + ": " + f.in + " or " + f.out + " is NULL");
    if ((rc = query_enter(ctx))) return rc;
    return staged_chunks(ctx, f, in, 0, out, count, segments, run);
}

// The run of a path family (run_radiance, run_gather, run_probe_sh) with a call's scalars bound.
template <class PathRun>
static auto bind_path_run(PathRun run, rt_ctx* ctx, uint32_t bounces, uint32_t first_sample, uint32_t samples) {
    return [=](const void* in, void* out, uint64_t n, unsigned long long* segs) {
        return run(ctx, in, out, n, bounces, first_sample, samples, segs);
    };
}

constexpr QueryFamily kTraceRays = {"rt_trace_rays", "rt_trace_rays_device", "rays", "hits", sizeof(rt_query_ray),
                                    sizeof(rt_hit), 16, 0, false};

int rt_trace_rays_device(rt_ctx* ctx, const void* rays_device, void* hits_device, uint64_t count) {
    return device_query(ctx, kTraceRays, rays_device, hits_device, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_query(ctx, in, out, n); });
}

int rt_trace_rays(rt_ctx* ctx, const rt_query_ray* rays, rt_hit* hits, uint64_t count) {
    return staged_query(ctx, kTraceRays, rays, hits, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_query(ctx, in, out, n); });
}

// The un-jittered camera ray of pixel (x, y), as the kernels read or compute it (pixel_ray), into the
// record at device pointer `d_ray` (it carries no t_max: the hit-list kernel takes +inf).
static int stage_pick_ray(rt_ctx* ctx, uint32_t x, uint32_t y, void* d_ray) {
    KernelArgs ka{};
    scene_base_args(ctx, ka);
    ka.camera_rays = ctx->d_rays;
    RT_HIP(ctx, rt_launch_pick_ray(ka, x, y, d_ray, ctx->stream));
    return RT_OK;
}

int rt_pick(rt_ctx* ctx, uint32_t x, uint32_t y, rt_hit* hit) {
    RT_ENTER_NOFLUSH(ctx);
    if (!hit) return fail(ctx, RT_E_INVALID, "rt_pick: hit is NULL");
    if (x >= ctx->width || y >= ctx->height) return fail(ctx, RT_E_INVALID, "rt_pick: pixel outside the framebuffer");
    int rc = query_enter(ctx);
    if (rc) return rc;
    if ((rc = query_buffers(ctx, 1))) return rc;
    unsigned char* d_ray = static_cast<unsigned char*>(ctx->d_query_buf);
    unsigned char* d_hit = d_ray + ctx->query_buf_rays * sizeof(rt_query_ray);
    if ((rc = stage_pick_ray(ctx, x, y, d_ray)) || (rc = run_query(ctx, d_ray, d_hit, 1))) return rc;
    unsigned char* h_hit = static_cast<unsigned char*>(ctx->query_pinned);
    RT_HIP(ctx, hipMemcpyAsync(h_hit, d_hit, sizeof(rt_hit), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(hit, h_hit, sizeof(rt_hit));
    return RT_OK;
}

// ---- occlusion queries (occlusion.hip) ---------------------------------------------------------
//
// The any-hit counterpart of the calls above, with the same scene visibility and the same absence
// of side effects; rt_occluded stages through the same buffers (32 B in, 1 B out per ray: the
// bytes go where the records of a closest-hit chunk would).
constexpr QueryFamily kOccluded = {"rt_occluded", "rt_occluded_device", "rays", "occluded", sizeof(rt_occlusion_ray),
                                   1, 1, 0, false};

int rt_occluded_device(rt_ctx* ctx, const void* rays_device, void* occluded_device, uint64_t count) {
    return device_query(ctx, kOccluded, rays_device, occluded_device, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_query(ctx, in, out, n, true); });
}

int rt_occluded(rt_ctx* ctx, const rt_occlusion_ray* rays, uint8_t* occluded, uint64_t count) {
    return staged_query(ctx, kOccluded, rays, occluded, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_query(ctx, in, out, n, true); });
}

// ---- hit-list queries (hits.hip) ---------------------------------------------------------------
//
// The K nearest hits of each ray, with the scene visibility and the absence of side effects of the
// calls above: `count` rt_occlusion_ray at device pointer `rays` into count x max_hits rt_hit at
// `hits` and, unless null, one count per ray at `counts`. `pick`: the rays are rt_pick's (no t_max).
static int run_hits(rt_ctx* ctx, const void* rays, void* hits, void* counts, uint64_t count, uint32_t max_hits,
                    bool pick = false) {
    if (count == 0) return RT_OK;
    QueryLaunch q;
    const int rc = query_scene(ctx, count, kQueryHits, q);
    if (rc) return rc;
    // every chunk from the counter, as the closest-hit kernel takes them
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident, 0u, rtq::kWalkChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    const hipError_t e = rt_launch_hits(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, rays, hits, counts, count, max_hits,
                                        pick, ctx->d_query_next, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_hits_kernel launch", e);
    return RT_OK;
}

// The check on max_hits, which comes first: an entry point refuses it whatever `count` is.
static int check_max_hits(rt_ctx* ctx, const char* entry, uint32_t max_hits) {
    if (max_hits == 0 || max_hits > RT_HITS_MAX)
        return fail(ctx, RT_E_INVALID, std::string(entry) + ": max_hits must be in [1, " + std::to_string(RT_HITS_MAX) + "]");
    return RT_OK;
}

int rt_trace_hits_device(rt_ctx* ctx, const void* rays_device, void* hits_device, void* counts_device, uint64_t count,
                         uint32_t max_hits) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_max_hits(ctx, "rt_trace_hits_device", max_hits);
    if (rc || count == 0) return rc;
    rc = check_device_ptrs(ctx, "rt_trace_hits_device",
                           {{rays_device, "rays", 16, false}, {hits_device, "hits", 16, false}, {counts_device, "counts", 4, true}});
    if (rc || (rc = query_enter(ctx))) return rc;
    return run_hits(ctx, rays_device, hits_device, counts_device, count, max_hits);
}

// Staged through the buffers of rt_trace_rays in chunks of max(1, query_chunk / max_hits) rays: a
// chunk's rays at the base, then its records, then its counts.
int rt_trace_hits(rt_ctx* ctx, const rt_occlusion_ray* rays, rt_hit* hits, uint32_t* counts, uint64_t count,
                  uint32_t max_hits) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_max_hits(ctx, "rt_trace_hits", max_hits);
    if (rc || count == 0) return rc;
    if (!rays || !hits) return fail(ctx, RT_E_INVALID, "rt_trace_hits: rays or hits is NULL");
    if ((rc = query_enter(ctx))) return rc;
    const size_t chunk = (size_t)std::min<uint64_t>(count, std::max<uint32_t>(1u, ctx->query_chunk / max_hits));
    const size_t ray_bytes = sizeof(rt_occlusion_ray), list_bytes = (size_t)max_hits * sizeof(rt_hit);
    // (a scratch "ray" is 96 bytes: chunk x max_hits of them hold the records, chunk more the rays and counts)
    if ((rc = query_buffers(ctx, chunk * max_hits + chunk))) return rc;
    unsigned char* d_in = static_cast<unsigned char*>(ctx->d_query_buf);
    unsigned char* h_in = static_cast<unsigned char*>(ctx->query_pinned);
    const size_t hits_at = chunk * ray_bytes, counts_at = hits_at + chunk * list_bytes;
    for (uint64_t done = 0; done < count;) {
        const size_t n = (size_t)std::min<uint64_t>(chunk, count - done);
        std::memcpy(h_in, rays + done, n * ray_bytes);
        RT_HIP(ctx, hipMemcpyAsync(d_in, h_in, n * ray_bytes, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = run_hits(ctx, d_in, d_in + hits_at, d_in + counts_at, n, max_hits))) return rc;
        RT_HIP(ctx, hipMemcpyAsync(h_in + hits_at, d_in + hits_at, n * list_bytes, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipMemcpyAsync(h_in + counts_at, d_in + counts_at, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(hits + done * max_hits, h_in + hits_at, n * list_bytes);
        if (counts) std::memcpy(counts + done, h_in + counts_at, n * sizeof(uint32_t));
        done += n;
    }
    return RT_OK;
}

int rt_pick_hits(rt_ctx* ctx, uint32_t x, uint32_t y, rt_hit* hits, uint32_t* n, uint32_t max_hits) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_max_hits(ctx, "rt_pick_hits", max_hits);
    if (rc) return rc;
    if (!hits || !n) return fail(ctx, RT_E_INVALID, "rt_pick_hits: hits or n is NULL");
    if (x >= ctx->width || y >= ctx->height)
        return fail(ctx, RT_E_INVALID, "rt_pick_hits: pixel outside the framebuffer");
    if ((rc = query_enter(ctx)) || (rc = query_buffers(ctx, (size_t)max_hits + 1u))) return rc;
    unsigned char* d_ray = static_cast<unsigned char*>(ctx->d_query_buf);
    const size_t hits_at = sizeof(rt_query_ray), list_bytes = (size_t)max_hits * sizeof(rt_hit);
    if ((rc = stage_pick_ray(ctx, x, y, d_ray)) ||
        (rc = run_hits(ctx, d_ray, d_ray + hits_at, d_ray + hits_at + list_bytes, 1, max_hits, true)))
        return rc;
    unsigned char* h_out = static_cast<unsigned char*>(ctx->query_pinned);
    RT_HIP(ctx, hipMemcpyAsync(h_out, d_ray + hits_at, list_bytes + sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(hits, h_out, list_bytes);
    std::memcpy(n, h_out + list_bytes, sizeof(uint32_t));
    return RT_OK;
}

// ---- proximity queries (nearest.hip) -----------------------------------------------------------
//
// Per point the closest surface point under THE NEAREST-POINT CONTRACT (include/rt_abi.h), with
// the scene visibility and the absence of side effects of the calls above.

// The table of |radius| as uploaded, by original sphere index, that the kernel's keys read (the
// slots hold radius * radius): rewritten after every sphere upload, and after a rebuild of the
// slots for another sphere count (it holds the first slots_count spheres of h_sph).
static int refresh_near_radius(rt_ctx* ctx) {
    const uint32_t n = ctx->slots_count == 0xffffffffu ? 0u : ctx->slots_count;
    if (ctx->d_near_radius && !ctx->near_radius_dirty) return RT_OK;
    int rc = grow_buffer(ctx, "nearest radii", &ctx->d_near_radius, &ctx->near_radius_bytes,
                         (size_t)std::max<uint32_t>(ctx->cap_sph, 1u) * sizeof(float));
    if (rc) return rc;
    std::vector<float> r(n);
    for (uint32_t i = 0; i < n; i++) r[i] = std::fabs(ctx->h_sph[i].radius);
    if ((rc = upload_raw(ctx, ctx->d_near_radius, r.data(), (size_t)n * sizeof(float)))) return rc;
    ctx->near_radius_dirty = false;
    return RT_OK;
}

// Whether the walk may cull by the triangle accelerator's boxes: every non-empty sub-object box
// that the sweep visits encloses a, fl(a + ab) and fl(a + ac) of its triangles within the margin,
// and no triangle in a finite box has a non-finite component (rtn::box_holds_triangle). One pass
// over the device's sub-objects and triangles, read back: the first query after a triangle,
// sub-object or object-range upload or a device edit copies every triangle to the host and waits
// for the stream, the device form included.
static int vouch_near_boxes(rt_ctx* ctx) {
    if (ctx->near_boxes != kNearBoxesUnknown) return RT_OK;
    int rc = sync_host_geometry(ctx);
    if (rc) return rc;
    const uint32_t n_tri = ctx->n_tri_dev;
    std::vector<RtTriangleHot> hot(n_tri);
    RT_HIP(ctx, hipMemcpyAsync(hot.data(), ctx->d_tri, (size_t)n_tri * sizeof(RtTriangleHot), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    bool ok = true;
    for (size_t o = 0; o < ctx->h_obj.size() && ok; o++) {
        const rt_object_info& ob = ctx->h_obj[o];
        for (uint32_t i = 0; i < ob.sub_object_count && ok; i++) {
            const size_t si = (size_t)ob.first_sub_object_index + i;
            if (si >= ctx->h_sub.size()) break;  // validated on upload; never taken
            const rt_sub_object_info& sub = ctx->h_sub[si];
            for (uint32_t j = 0; j < sub.triangle_count && ok; j++) {
                const size_t ti = (size_t)sub.first_triangle_index + j;
                if (ti >= n_tri) {  // the kernel clamps the index: another sub-object's triangle
                    ok = false;
                    break;
                }
                float a[3], ab[3], ac[3], cn[3], fn[3];
                unpack_triangle(hot[ti], a, ab, ac, cn, fn);
                ok = rtn::box_holds_triangle(sub.min_bounds, sub.max_bounds, rtn::v3(a[0], a[1], a[2]),
                                             rtn::v3(ab[0], ab[1], ab[2]), rtn::v3(ac[0], ac[1], ac[2]));
            }
        }
    }
    ctx->near_boxes = ok ? kNearBoxesVouched : kNearBoxesRefuted;
    return RT_OK;
}

// Answers `count` rt_near_point at device pointer `points` into rt_nearest records at `out`,
// stream-ordered on the primary stream. The sweep instance runs in brute-force mode, with tuning
// "nearest_walk" 0, and while the sub-object boxes are not vouched for; "nearest_walk" 2 is the walk
// without its greedy descent.
static int run_nearest(rt_ctx* ctx, const void* points, void* out, uint64_t count) {
    if (count == 0) return RT_OK;
    int rc = refresh_near_radius(ctx);
    if (rc) return rc;
    bool sweep = ctx->brute != 0 || ctx->nearest_walk == 0;
    if (!sweep && ctx->params.object_count != 0 && ctx->use_tri_bvh) {
        if ((rc = vouch_near_boxes(ctx))) return rc;
        sweep = ctx->near_boxes != kNearBoxesVouched;
    }
    QueryLaunch q;
    if ((rc = query_scene(ctx, count, sweep ? kQueryNearestSweep : kQueryNearest, q))) return rc;
    // every chunk from the counter, as the closest-hit kernel takes them
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident, 0u, rtq::kWalkChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    const hipError_t e = rt_launch_nearest(q.ka, q.sl.mode, q.sl.tris, sweep, q.lds_bytes, s, points, out,
                                           ctx->d_near_radius, ctx->nearest_walk == 1, count, ctx->d_query_next,
                                           ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_nearest_kernel launch", e);
    return RT_OK;
}

static_assert(sizeof(rt_near_point) == 16 && sizeof(struct rt_nearest) == 64, "proximity record layouts");
constexpr QueryFamily kNearest = {"rt_nearest", "rt_nearest_device", "points", "out", sizeof(rt_near_point),
                                  sizeof(struct rt_nearest), 16, 0, false};

int rt_nearest_device(rt_ctx* ctx, const void* points_device, void* out_device, uint64_t count) {
    return device_query(ctx, kNearest, points_device, out_device, count, 0, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) { return run_nearest(ctx, in, out, n); });
}

int rt_nearest(rt_ctx* ctx, const rt_near_point* points, struct rt_nearest* out, uint64_t count) {
    return staged_query(ctx, kNearest, points, out, count, 0, nullptr,
                        [=](const void* in, void* d_out, uint64_t n, unsigned long long*) { return run_nearest(ctx, in, d_out, n); });
}

// ---- radiance queries (radiance.hip) -----------------------------------------------------------
//
// per_pixel for arbitrary rays, with the scene visibility and the absence of side effects of the
// calls above. rt_radiance stages through the same buffers (32 B in, 16 B out per ray: the sums go
// where the records of a closest-hit chunk would).

// The answer of a path query of zero bounces, `out_bytes` per record: the bounce loop does not run
// (:226), so there is no light and there are no segments.
static int answer_zero_bounces(rt_ctx* ctx, void* out, uint64_t count, size_t out_bytes) {
    RT_HIP(ctx, hipMemsetAsync(out, 0, (size_t)count * out_bytes, ctx->stream));
    return RT_OK;
}

// The walks of `count` records of `samples` each, for the placement threshold of the other queries.
static uint64_t query_walks(uint64_t count, uint32_t samples) {
    return count > UINT64_MAX / samples ? UINT64_MAX : count * samples;
}

// The head of a radiance, gather or probe launch (`kind`) of `count` records, `bounces` > 0: `q`
// receives the scene view, placed by the walks the call runs at least, and the shading arguments.
static int path_query_scene(rt_ctx* ctx, uint64_t count, uint32_t bounces, uint32_t samples, int kind, QueryLaunch& q) {
    const int rc = query_scene(ctx, query_walks(count, samples), kind, q);
    if (rc) return rc;
    q.ka.bounces = bounces;
    q.ka.drain_threshold = ctx->drain_threshold;
    q.ka.drain_min_steps = ctx->drain_min_steps;
    return RT_OK;
}

// Path-traces `count` rays at device pointer `rays` into `radiance`, stream-ordered on the primary
// stream; the batch's counted segments are added to the device counter `segments` (null: not
// counted).
static int run_radiance(rt_ctx* ctx, const void* rays, void* radiance, uint64_t count, uint32_t bounces,
                        uint32_t first_sample, uint32_t samples, unsigned long long* segments) {
    if (count == 0) return RT_OK;
    if (bounces == 0) return answer_zero_bounces(ctx, radiance, count, 16u);
    QueryLaunch q;
    const int rc = path_query_scene(ctx, count, bounces, samples, kQueryRadiance, q);
    if (rc) return rc;
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident, rtq::kRadianceFirstChunkMax,
                                                     rtq::kRadianceChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    const hipError_t e = rt_launch_radiance(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, rays, radiance, count,
                                            ctx->d_query_next, segments, first_sample, samples, 0u, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_radiance_kernel launch", e);
    return RT_OK;
}

constexpr QueryFamily kRadiance = {"rt_radiance", "rt_radiance_device", "rays", "radiance", sizeof(rt_radiance_ray),
                                   16, 16, kAnySamples, true};

int rt_radiance_device(rt_ctx* ctx, const void* rays_device, void* radiance_device, uint64_t count, uint32_t bounces,
                       uint32_t first_sample, uint32_t samples, void* segments_device) {
    return device_query(ctx, kRadiance, rays_device, radiance_device, count, samples, segments_device,
                        bind_path_run(run_radiance, ctx, bounces, first_sample, samples));
}

int rt_radiance(rt_ctx* ctx, const rt_radiance_ray* rays, float* radiance, uint64_t count, uint32_t bounces,
                uint32_t first_sample, uint32_t samples, uint64_t* segments) {
    return staged_query(ctx, kRadiance, rays, radiance, count, samples, segments,
                        bind_path_run(run_radiance, ctx, bounces, first_sample, samples));
}

// ---- gather queries (radiance.hip, kGather) -----------------------------------------------------
//
// Per point, the tree-reduced light of `samples` paths through the diffuse lobe (the contract in
// include/rt_abi.h). The path kernel is the radiance kernel's gather instance over (point, stripe)
// items; rt_gather_resolve_kernel reduces each point's partials.

// The launches of a gather or an ambient call, which differ in their kernel: `count` points (32-byte
// records) at device pointer `points` in launches of at most "gather_chunk" points, each
// launch(schedule, its points, items, stripes) over (point, stripe) items into the context's
// partials, which rt_gather_resolve_kernel reduces into `out`. `what` names the launch in an error.
template <class Launch>
static int run_striped(rt_ctx* ctx, const QueryLaunch& q, const void* points, void* out, uint64_t count,
                       uint32_t samples, const char* what, Launch launch) {
    const uint32_t stripes = std::min<uint32_t>(samples, 64u);
    const uint64_t chunk = std::min<uint64_t>(count, ctx->gather_chunk);
    const int rc = grow_buffer(ctx, "gather partials", &ctx->d_gather_partials, &ctx->gather_partials_bytes, (size_t)chunk * 1024u);
    if (rc) return rc;
    for (uint64_t done = 0; done < count;) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, count - done);
        // the launch is sized by its items, (point, stripe) pairs: at most 2^20 x 64
        const uint64_t items = (uint64_t)n * stripes;
        const rtq::QuerySchedule s = rtq::query_schedule(items, q.waves_per_block, q.resident,
                                                         rtq::kRadianceFirstChunkMax, rtq::kRadianceChunkMax);
        RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
        hipError_t e = launch(s, static_cast<const unsigned char*>(points) + done * sizeof(rt_gather_point), items, stripes);
        if (e != hipSuccess) return hip_fail(ctx, what, e);
        e = rt_launch_gather_resolve(ctx->d_gather_partials, static_cast<unsigned char*>(out) + done * 16u, n, stripes,
                                     ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, "rt_gather_resolve_kernel launch", e);
        done += n;
    }
    return RT_OK;
}

// Gathers at `count` points at device pointer `points` into `radiance`, stream-ordered on the
// primary stream, in launches of at most "gather_chunk" points; the counted segments are added to
// the device counter `segments` (null: not counted).
static int run_gather(rt_ctx* ctx, const void* points, void* radiance, uint64_t count, uint32_t bounces,
                      uint32_t first_sample, uint32_t samples, unsigned long long* segments) {
    if (count == 0) return RT_OK;
    if (bounces == 0) return answer_zero_bounces(ctx, radiance, count, 16u);
    QueryLaunch q;
    const int rc = path_query_scene(ctx, count, bounces, samples, kQueryGather, q);
    if (rc) return rc;
    return run_striped(ctx, q, points, radiance, count, samples, "rt_radiance_kernel (gather) launch",
                       [&](const rtq::QuerySchedule& s, const void* records, uint64_t items, uint32_t stripes) {
                           return rt_launch_radiance(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, records,
                                                     ctx->d_gather_partials, items, ctx->d_query_next, segments,
                                                     first_sample, samples, stripes, ctx->stream);
                       });
}

constexpr QueryFamily kGather = {"rt_gather", "rt_gather_device", "points", "radiance", sizeof(rt_gather_point),
                                 16, 16, kAnySamples, true};

int rt_gather_device(rt_ctx* ctx, const void* points_device, void* radiance_device, uint64_t count, uint32_t bounces,
                     uint32_t first_sample, uint32_t samples, void* segments_device) {
    return device_query(ctx, kGather, points_device, radiance_device, count, samples, segments_device,
                        bind_path_run(run_gather, ctx, bounces, first_sample, samples));
}

int rt_gather(rt_ctx* ctx, const rt_gather_point* points, float* radiance, uint64_t count, uint32_t bounces,
              uint32_t first_sample, uint32_t samples, uint64_t* segments) {
    return staged_query(ctx, kGather, points, radiance, count, samples, segments,
                        bind_path_run(run_gather, ctx, bounces, first_sample, samples));
}

// ---- ambient queries (ambient.hip) ---------------------------------------------------------------
//
// Per point, the open count and the sum of the open directions among `samples` any-hit searches
// through the gather's lobe (the contract in include/rt_abi.h), with the scene visibility and the
// absence of side effects of rt_occluded. rt_ambient_kernel runs (point, stripe) items into the
// gather's partials; rt_gather_resolve_kernel reduces each point's partials.

// The most samples per point: `open` stays an exactly represented integer (2^24).
constexpr uint32_t kMaxAmbientSamples = 1u << 24;

// Answers `count` points at device pointer `points` into `out`, stream-ordered on the primary
// stream, in launches of at most "gather_chunk" points.
static int run_ambient(rt_ctx* ctx, const void* points, void* out, uint64_t count, uint32_t first_sample,
                       uint32_t samples) {
    if (count == 0) return RT_OK;
    QueryLaunch q;
    // the placement threshold of the other queries, on the walks the call runs at most
    const int rc = query_scene(ctx, query_walks(count, samples), kQueryAmbient, q);
    if (rc) return rc;
    return run_striped(ctx, q, points, out, count, samples, "rt_ambient_kernel launch",
                       [&](const rtq::QuerySchedule& s, const void* records, uint64_t items, uint32_t stripes) {
                           return rt_launch_ambient(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, records,
                                                    ctx->d_gather_partials, items, ctx->d_query_next, first_sample,
                                                    samples, stripes, ctx->stream);
                       });
}

constexpr QueryFamily kAmbient = {"rt_ambient", "rt_ambient_device", "points", "out", sizeof(rt_ambient_point),
                                  16, 16, kMaxAmbientSamples, false};

int rt_ambient_device(rt_ctx* ctx, const void* points_device, void* out_device, uint64_t count, uint32_t first_sample,
                      uint32_t samples) {
    return device_query(ctx, kAmbient, points_device, out_device, count, samples, nullptr,
                        [=](const void* in, void* out, uint64_t n, unsigned long long*) {
                            return run_ambient(ctx, in, out, n, first_sample, samples);
                        });
}

int rt_ambient(rt_ctx* ctx, const rt_ambient_point* points, float* out, uint64_t count, uint32_t first_sample,
               uint32_t samples) {
    return staged_query(ctx, kAmbient, points, out, count, samples, nullptr,
                        [=](const void* d_in, void* d_out, uint64_t n, unsigned long long*) {
                            return run_ambient(ctx, d_in, d_out, n, first_sample, samples);
                        });
}

// ---- probe queries (radiance.hip, kPathProbe) ---------------------------------------------------
//
// Per probe, the second-order spherical-harmonic projection of the light of `samples` paths that
// leave the point in uniform directions (the contract in include/rt_abi.h). The path kernel is the
// radiance kernel's probe instance over (probe, sample) items, which stores every path's light;
// rt_probe_resolve_kernel projects and reduces each probe's lights.

// Bakes `count` probes at device pointer `probes` into `sh`, stream-ordered on the primary stream,
// in launches of whole probes, max(1, "probe_chunk" / samples) of them, two of them in flight (the
// primary stream is ordered after both on return); the counted segments are added to the device
// counter `segments` (null: not counted).
static int run_probe_sh(rt_ctx* ctx, const void* probes, void* sh, uint64_t count, uint32_t bounces,
                        uint32_t first_sample, uint32_t samples, unsigned long long* segments) {
    if (count == 0) return RT_OK;
    if (bounces == 0) return answer_zero_bounces(ctx, sh, count, 144u);
    QueryLaunch q;
    int rc = path_query_scene(ctx, count, bounces, samples, kQueryProbe, q);
    if (rc) return rc;
    // whole probes per launch: at most max("probe_chunk", samples) <= 2^26 items, 16 B each
    const uint64_t chunk = std::min<uint64_t>(count, std::max<uint32_t>(1u, ctx->probe_chunk / samples));
    const size_t bytes = (size_t)chunk * samples * 16u;
    // A call of several launches alternates them between the primary and the auxiliary stream, each
    // with its own half of the scratch and its own chunk counter: a launch of a million paths is
    // mostly fill and drain (four items per resident lane), and the next launch's workgroups take
    // the CUs the draining one gives up. Not where that would take the scratch beyond its cap.
    const bool overlap = count > chunk && 2u * bytes <= kMaxProbeScratchBytes;
    if ((rc = grow_buffer(ctx, "probe lights", &ctx->d_probe_lights, &ctx->probe_lights_bytes, overlap ? 2u * bytes : bytes))) return rc;
    if (overlap) {
        if (!ctx->d_probe_next && (rc = dev_alloc(ctx, &ctx->d_probe_next, 2))) return rc;
        RT_HIP(ctx, hipEventRecord(ctx->ev_primary, ctx->stream));  // the probes are there, the scratch is free
        RT_HIP(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->ev_primary, 0));
    }
    // orders the primary stream after the auxiliary one again (on every way out)
    auto join = [&]() -> hipError_t {
        if (!overlap) return hipSuccess;
        const hipError_t e = hipEventRecord(ctx->ev_aux_done, ctx->aux_stream);
        if (e != hipSuccess) return e;
        ctx->aux_outstanding = true;
        return join_aux(ctx);
    };
    uint32_t group = 0;
    for (uint64_t done = 0; done < count; ++group) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, count - done);
        const uint64_t items = (uint64_t)n * samples;
        const rtq::QuerySchedule s = rtq::query_schedule(items, q.waves_per_block, q.resident,
                                                         rtq::kRadianceFirstChunkMax, rtq::kRadianceChunkMax);
        const uint32_t slot = overlap ? group & 1u : 0u;
        hipStream_t S = slot ? ctx->aux_stream : ctx->stream;
        unsigned long long* next = overlap ? ctx->d_probe_next + slot : ctx->d_query_next;
        unsigned char* lights = static_cast<unsigned char*>(ctx->d_probe_lights) + slot * bytes;
        const unsigned char* records = static_cast<const unsigned char*>(probes) + done * sizeof(rt_probe);
        hipError_t e = hipMemsetAsync(next, 0, sizeof(unsigned long long), S);
        if (e == hipSuccess)
            e = rt_launch_probe_paths(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, records, lights, items, next, segments,
                                      first_sample, samples, S);
        if (e == hipSuccess)
            e = rt_launch_probe_resolve(lights, records, static_cast<unsigned char*>(sh) + done * 144u, n, first_sample,
                                        samples, S);
        if (e != hipSuccess) {
            (void)join();
            return hip_fail(ctx, "rt_probe_sh launch", e);
        }
        done += n;
    }
    RT_HIP(ctx, join());
    return RT_OK;
}

constexpr QueryFamily kProbeSh = {"rt_probe_sh", "rt_probe_sh_device", "probes", "sh", sizeof(rt_probe),
                                  144, 16, kMaxProbeSamples, true};

int rt_probe_sh_device(rt_ctx* ctx, const void* probes_device, void* sh_device, uint64_t count, uint32_t bounces,
                       uint32_t first_sample, uint32_t samples, void* segments_device) {
    return device_query(ctx, kProbeSh, probes_device, sh_device, count, samples, segments_device,
                        bind_path_run(run_probe_sh, ctx, bounces, first_sample, samples));
}

int rt_probe_sh(rt_ctx* ctx, const rt_probe* probes, float* sh, uint64_t count, uint32_t bounces, uint32_t first_sample,
                uint32_t samples, uint64_t* segments) {
    return staged_query(ctx, kProbeSh, probes, sh, count, samples, segments,
                        bind_path_run(run_probe_sh, ctx, bounces, first_sample, samples));
}

// ---- lens queries (radiance.hip, kPathLens) -----------------------------------------------------
//
// Per pixel of a range of the descriptor's image, the summed light of `samples` paths whose first
// ray is drawn on the device from the descriptor (the contract in include/rt_abi.h). The path
// kernel is the radiance kernel's lens instance over the range's pixels; rt_lens_rays_kernel writes
// the same rays as records. The launches read the descriptor from the context's copy
// (d_lens_cam), which rt_lens_store_kernel writes on the primary stream from a kernel argument:
// every lens launch runs on that stream too, so the copy changes only after the launches that read
// the earlier one and before those that follow, whatever the host does in between. (The chunks of
// a host form share the copy of their call; the auxiliary stream runs no lens launch.)

constexpr QueryFamily kLens = {"rt_lens", "rt_lens_device", "cam", "radiance", 0, 16, 16, kAnySamples, true};
constexpr QueryFamily kLensRays = {"rt_lens_rays", "rt_lens_rays_device", "cam", "rays", 0, 32, 16, 0, false};

// Consequence 6 of the lens contract, for the range [first_pixel, first_pixel + count), count > 0.
static int check_lens(rt_ctx* ctx, const char* entry, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count) {
    auto bad = [&](const char* why) { return fail(ctx, RT_E_INVALID, std::string(entry) + ": " + why); };
    if (!cam) return bad("cam is NULL");
    if (cam->kind > RT_LENS_EQUIRECT) return bad("unknown kind");
    if (cam->width == 0 || cam->height == 0) return bad("width or height is 0");
    const uint64_t pixels = (uint64_t)cam->width * cam->height;  // (below 2^64)
    if (pixels > (1ull << 32)) return bad("width * height above 2^32");
    if (first_pixel > pixels || count > pixels - first_pixel) return bad("the range lies outside the image");
    if (!(cam->aperture >= 0.0f) || std::isinf(cam->aperture)) return bad("aperture is negative or not finite");
    if (cam->kind == RT_LENS_PERSPECTIVE && cam->aperture > 0.0f && !(cam->focus > 0.0f))
        return bad("focus must be > 0 when aperture > 0");
    if (cam->kind == RT_LENS_ORTHOGRAPHIC && !(cam->ortho_half_height > 0.0f)) return bad("ortho_half_height must be > 0");
    return RT_OK;
}

// The context's copy of `cam` for the launches that follow on the primary stream.
static int stage_lens_camera(rt_ctx* ctx, const rt_lens_camera* cam) {
    if (!ctx->d_lens_cam) {
        const int rc = dev_alloc(ctx, &ctx->d_lens_cam, sizeof(rt_lens_camera) / sizeof(uint4));
        if (rc) return rc;
    }
    const hipError_t e = rt_launch_lens_camera(*cam, ctx->d_lens_cam, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_lens_store_kernel launch", e);
    return RT_OK;
}

// Path-traces the `count` pixels from `first_pixel` on of the staged descriptor's image into
// `radiance`, stream-ordered on the primary stream; the counted segments are added to the device
// counter `segments` (null: not counted).
static int run_lens(rt_ctx* ctx, uint64_t first_pixel, void* radiance, uint64_t count, uint32_t bounces,
                    uint32_t first_sample, uint32_t samples, unsigned long long* segments) {
    if (count == 0) return RT_OK;
    if (bounces == 0) return answer_zero_bounces(ctx, radiance, count, 16u);
    QueryLaunch q;
    const int rc = path_query_scene(ctx, count, bounces, samples, kQueryLens, q);
    if (rc) return rc;
    const rtq::QuerySchedule s = rtq::query_schedule(count, q.waves_per_block, q.resident, rtq::kRadianceFirstChunkMax,
                                                     rtq::kRadianceChunkMax);
    RT_HIP(ctx, hipMemsetAsync(ctx->d_query_next, 0, sizeof(unsigned long long), ctx->stream));
    // (first_pixel < width * height <= 2^32 with count > 0: check_lens)
    const hipError_t e = rt_launch_lens(q.ka, q.sl.mode, q.sl.tris, q.lds_bytes, s, ctx->d_lens_cam, radiance,
                                        (uint32_t)first_pixel, count, ctx->d_query_next, segments, first_sample,
                                        samples, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_radiance_kernel (lens) launch", e);
    return RT_OK;
}

int rt_lens_device(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count, void* radiance_device,
                   uint32_t bounces, uint32_t first_sample, uint32_t samples, void* segments_device) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_samples(ctx, kLens, kLens.device, samples);
    if (rc || count == 0) return rc;
    if ((rc = check_lens(ctx, kLens.device, cam, first_pixel, count))) return rc;
    rc = check_device_ptrs(ctx, kLens.device, {{radiance_device, kLens.out, 16, false}, {segments_device, "segments", 8, true}});
    if (rc || (rc = query_enter(ctx)) || (rc = stage_lens_camera(ctx, cam))) return rc;
    return run_lens(ctx, first_pixel, radiance_device, count, bounces, first_sample, samples,
                    static_cast<unsigned long long*>(segments_device));
}

int rt_lens(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count, float* radiance,
            uint32_t bounces, uint32_t first_sample, uint32_t samples, uint64_t* segments) {
    RT_ENTER_NOFLUSH(ctx);
    int rc = check_samples(ctx, kLens, kLens.host, samples);
    if (rc) return rc;
    if (count == 0) {
        if (segments) *segments = 0;
        return RT_OK;
    }
    if ((rc = check_lens(ctx, kLens.host, cam, first_pixel, count))) return rc;
    if (!radiance) return fail(ctx, RT_E_INVALID, "rt_lens: radiance is NULL");
    if ((rc = query_enter(ctx)) || (rc = stage_lens_camera(ctx, cam))) return rc;
    return staged_chunks(ctx, kLens, nullptr, first_pixel, radiance, count, segments,
                         [=](uint64_t first, void* out, uint64_t n, unsigned long long* segs) {
                             return run_lens(ctx, first, out, n, bounces, first_sample, samples, segs);
                         });
}

// The records of the range's rays (steps A to D for the sample index u): no scene, nothing but the
// descriptor is read.
static int run_lens_rays(rt_ctx* ctx, uint64_t first_pixel, void* rays, uint64_t count, uint32_t u) {
    const hipError_t e = rt_launch_lens_rays(ctx->d_lens_cam, rays, (uint32_t)first_pixel, count, u, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "rt_lens_rays_kernel launch", e);
    return RT_OK;
}

int rt_lens_rays_device(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count,
                        uint32_t sample_index, void* rays_device) {
    RT_ENTER_NOFLUSH(ctx);
    if (count == 0) return RT_OK;
    int rc = check_lens(ctx, kLensRays.device, cam, first_pixel, count);
    if (rc) return rc;
    rc = check_device_ptrs(ctx, kLensRays.device, {{rays_device, kLensRays.out, 16, false}});
    if (rc || (rc = stage_lens_camera(ctx, cam))) return rc;
    return run_lens_rays(ctx, first_pixel, rays_device, count, sample_index);
}

int rt_lens_rays(rt_ctx* ctx, const rt_lens_camera* cam, uint64_t first_pixel, uint64_t count, uint32_t sample_index,
                 rt_radiance_ray* rays) {
    RT_ENTER_NOFLUSH(ctx);
    if (count == 0) return RT_OK;
    int rc = check_lens(ctx, kLensRays.host, cam, first_pixel, count);
    if (rc) return rc;
    if (!rays) return fail(ctx, RT_E_INVALID, "rt_lens_rays: rays is NULL");
    if ((rc = stage_lens_camera(ctx, cam))) return rc;
    return staged_chunks(ctx, kLensRays, nullptr, first_pixel, rays, count, nullptr,
                         [=](uint64_t first, void* out, uint64_t n, unsigned long long*) {
                             return run_lens_rays(ctx, first, out, n, sample_index);
                         });
}
