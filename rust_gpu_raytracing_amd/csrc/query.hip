// query.hip -- batched closest-hit ray queries for gfx950 (rt_trace_rays, rt_trace_rays_device,
// rt_pick).
//
// rt_query_kernel answers "what does this ray hit?" for arbitrary rays (o, d) with the search the
// path kernel runs for every path segment (rt_walk.h): trace_begin, the per-lane walk with deferred
// or cooperative leaf batches, trace_end. No shading, no RNG, nothing of the framebuffer is read
// or written. What is MI355X-specific:
//
//  * Each lane owns one ray. Persistent wave64s claim chunks of consecutive rays from one device
//    counter; lanes whose ray finishes take the chunk's next rays (ballot + mbcnt, a wave-wide
//    prefix sum over the idle lanes), so a wave does not idle behind one long walk. This frame,
//    which the occlusion and radiance kernels stand on too, is rt_query_frame.h.
//  * A ray is read with two 16-B loads (rt_query_ray, 32 B) and its record written with four 16-B
//    stores (rt_hit, 64 B): a wave's finished lanes write whole 64-B segments.
//  * Scene placement is the path kernel's: mode 0 reads everything from global memory (no staging:
//    what small batches launch), mode 1 stages spheres / objects / the sphere BVH in LDS once per
//    workgroup, mode 2 also the triangle accelerator. Every mode returns the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rt_launch.h"
#include "rt_path_common.h"
#include "rt_query_frame.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

using namespace rtk;

struct QueryArgs {
    const float4* __restrict__ rays;  // rt_query_ray[count]: {origin.xyz, pad}, {direction.xyz, pad}
    uint4* __restrict__ hits;         // rt_hit[count]
    ChunkArgs chunks;                 // every chunk is claimed: first_chunk and claimed_from are 0
};

namespace {

// The sub-object of object `obj` that holds triangle `tri`: the sweep's sub-objects of an object
// cover ascending triangle ranges (create_sub_objects), so a binary search over the object's
// records finds it in log2(n) loads -- cheaper than carrying it through every leaf test of the walk
// (one more live register per lane for a value only the final record needs). Ranges that are not
// ascending fall back to the first record in order that holds the triangle.
__device__ __forceinline__ uint32_t find_sub_object(const SceneView& sv, const KernelArgs& ka, uint32_t obj,
                                                    uint32_t tri) {
    const RtObject& ob = sv.obj[obj];
    const uint32_t first = ob.first_sub_object_index, n = ob.sub_object_count;
    const uint32_t last = ka.sub_object_count - 1u;
    if (n == 0u) return min(first, last);
    uint32_t lo = 0u, hi = n - 1u;  // the last record whose first triangle is <= tri
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (sv.sub[min(first + mid, last)].first_triangle_index <= tri)
            lo = mid;
        else
            hi = mid - 1u;
    }
    auto holds = [&](uint32_t i) {
        const RtSubObject& s = sv.sub[min(first + i, last)];
        return tri >= s.first_triangle_index && tri - s.first_triangle_index < s.triangle_count;
    };
    if (holds(lo)) return min(first + lo, last);
    for (uint32_t i = 0; i < n; ++i)
        if (holds(i)) return min(first + i, last);
    return min(first + lo, last);
}

}  // namespace

template <int kMode, bool kTris, uint32_t kThreads>
__global__ void __launch_bounds__(kThreads, 1) rt_query_kernel(KernelArgs ka, QueryArgs qa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // The part of the path kernel's LDS image the search and the record read (materials, their
    // glass constants and the sRGB table are shading's: left out).
    SceneView sv = global_scene_view<kMode, kTris>(ka, nullptr);
    if constexpr (kMode >= 1) {
        sv = stage_walk_tables<kTris, kThreads>(ka, lds, sv);
        sv = stage_sphere_materials<kThreads>(ka, lds, sv);
    }
    if constexpr (kMode == 2) sv = stage_triangle_tables<kThreads>(ka, lds, sv);
    if constexpr (kMode >= 1) __syncthreads();

    // Lane states. A lane owns one ray at a time.
    constexpr uint32_t kIdle = 0, kSetup = 1, kTrav = 2, kDone = 3;
    uint32_t mode = kIdle;
    unsigned long long ray = 0;
    f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
    TraceState ts = idle_trace_state(kF32Max);

    // No wave has a first chunk of its own here: every chunk comes from the counter.
    WaveChunk c{0, 0, false, false};
    claim_chunk<false>(qa.chunks, 0u, c);

    while (true) {
        // 1. The records of the lanes whose search has finished (trace_ray's result, :342-353).
        if (mode == kDone) {
            const Hit h = trace_end<kTris, true>(sv, ka, o, d, ts);
            const HitId id = trace_end_id<kTris>(ts);
            uint32_t sub = 0u;
            if constexpr (kTris)
                if (id.kind == 2u) sub = find_sub_object(sv, ka, id.index, id.triangle);
            uint4* rec = qa.hits + 4ull * ray;
            rec[0] = make_uint4(__float_as_uint(h.t), __float_as_uint(h.p.x), __float_as_uint(h.p.y),
                                __float_as_uint(h.p.z));
            rec[1] = make_uint4(__float_as_uint(h.n.x), __float_as_uint(h.n.y), __float_as_uint(h.n.z),
                                __float_as_uint(h.u));
            rec[2] = make_uint4(__float_as_uint(h.v), h.material_index, h.front_face ? 1u : 0u, id.kind);
            rec[3] = make_uint4(id.index, sub, id.triangle, 0u);
            mode = kIdle;
        }
        // 2. Refill: idle lanes take the chunk's next rays, in order.
        while (true) {
            const uint64_t need = __ballot(mode == kIdle);
            if (need == 0 || c.dry) break;
            const uint32_t avail = (uint32_t)(c.end - c.next);
            if (mode == kIdle) {
                const uint32_t rank = rank_among(need);
                if (rank < avail) {
                    ray = c.next + rank;
                    const float4 r0 = qa.rays[2ull * ray], r1 = qa.rays[2ull * ray + 1ull];
                    o = mk(r0.x, r0.y, r0.z);
                    d = mk(r1.x, r1.y, r1.z);
                    mode = kSetup;
                }
            }
            c.next += min((uint32_t)__popcll(need), avail);
            if (c.next == c.end) claim_chunk<false>(qa.chunks, 0u, c);
        }
        // 3. Start the search of every lane that took a ray.
        if (mode == kSetup) {
            trace_begin<kTris>(sv, ka, o, d, ts);
            mode = ts.phase == 2 ? kDone : kTrav;
        }
        if (__ballot(mode != kIdle) == 0 && c.dry) break;
        // 4. Traverse (query_traverse): finished lanes wait for the wave, which then writes their
        // records and refills them together; with no rays left it traverses to the end (a
        // finished ray has no next segment that an earlier return would start sooner).
        take_lane_walk(query_traverse<kMode, kTris, false>(sv, ka, o, d, lane_walk(ts, mode), c.dry, lds, WalkEnd{}),
                       ts, mode);
    }
}

// The instances, (mode, triangles, threads): f(kernel, threads) for the one of (mode, tris).
// Workgroup size by placement: the global-memory instance has no image to share, so small
// workgroups (more of them resident, started sooner); the staged instances share one image among
// 16 waves as the path kernel's largest workgroup does.
template <class F>
static hipError_t with_query_instance(int mode, bool tris, F f) {
    if (mode == 0 && tris) return f(&rt_query_kernel<0, true, 256>, 256u);
    if (mode == 1 && tris) return f(&rt_query_kernel<1, true, 1024>, 1024u);
    if (mode == 2 && tris) return f(&rt_query_kernel<2, true, 1024>, 1024u);
    if (mode == 0 && !tris) return f(&rt_query_kernel<0, false, 256>, 256u);
    if (mode == 1 && !tris) return f(&rt_query_kernel<1, false, 1024>, 1024u);
    return hipErrorInvalidValue;
}

// (0 for a (mode, tris) without an instance; its occupancy query fails too, and query_scene takes
// the next lower placement)
uint32_t rt_query_threads(int mode, bool tris) {
    uint32_t threads = 0;
    (void)with_query_instance(mode, tris, [&](auto, uint32_t t) { return threads = t, hipSuccess; });
    return threads;
}

hipError_t rt_query_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return with_query_instance(
        mode, tris, [&](auto kernel, uint32_t t) { return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu); });
}

hipError_t rt_launch_query(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                           const void* rays, void* hits, uint64_t count, unsigned long long* counter,
                           hipStream_t stream) {
    if (s.blocks == 0 || count == 0) return hipSuccess;
    return with_query_instance(mode, tris, [&](auto kernel, uint32_t t) {
        const QueryArgs qa{static_cast<const float4*>(rays), static_cast<uint4*>(hits), chunk_args(count, counter, s, t)};
        return query_launch_of(kernel, t, s.blocks, lds_bytes, stream, ka, qa);
    });
}

// rt_pick's ray: the pixel's un-jittered camera ray -- the camera origin and the direction the
// kernels read from the ray buffer or compute from the camera matrices (pixel_ray) -- as one
// rt_query_ray record.
__global__ void __launch_bounds__(64) rt_pick_ray_kernel(KernelArgs ka, uint32_t x, uint32_t y, float4* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float cam[33];
    for (int i = 0; i < 16; ++i) {
        cam[i] = ka.inv_proj[i];
        cam[16 + i] = ka.inv_view[i];
    }
    cam[32] = ka.aspect;
    const f3 d = pixel_ray(ka, cam, y * ka.width + x, x, y);
    out[0] = make_float4(ka.camera_origin[0], ka.camera_origin[1], ka.camera_origin[2], 0.0f);
    out[1] = make_float4(d.x, d.y, d.z, 0.0f);
}

hipError_t rt_launch_pick_ray(const KernelArgs& ka, uint32_t x, uint32_t y, void* ray_out, hipStream_t stream) {
    hipLaunchKernelGGL(rt_pick_ray_kernel, dim3(1), dim3(64), 0, stream, ka, x, y, static_cast<float4*>(ray_out));
    return hipGetLastError();
}
