// occlusion.hip -- batched any-hit ray queries for gfx950 (rt_occluded, rt_occluded_device;
// DESIGN.md §5.4c).
//
// rt_occlusion_kernel answers "is anything in the way before t_max?" for arbitrary rays: one byte
// per ray, 1 iff at least one primitive, tested on its own by the reference's test, is accepted at
// a non-NaN distance t < t_max. It stands on the query kernels' frame (rt_query_frame.h): one ray
// per lane, persistent wave64s taking chunks of rays (each wave's own first chunk, then claims from
// one device counter), ballot + mbcnt refill, the three scene placements, the walk of rt_walk.h.
// What differs from the closest-hit query (query.hip) -- the search itself (occlusion_begin,
// OccluderEnd, occluder_found) is rt_occlusion_walk.h's, which the ambient kernel shares:
//
//  * The bound is the search state's seed. Both running bests start at t_max instead of "none":
//    the walk's own acceptance rule (strictly closer than the best; an equal distance only with a
//    lower sweep position / sphere index, and the seed's is 0) then accepts exactly the candidates
//    with t < t_max, and every bound the closest-hit walk has proved for its best hit culls for
//    t_max from the first node: the sphere walk's prune_limit with its slack, and on the
//    global-memory triangle walk the leaf certificates (§5.3c). The LDS-resident triangle walk
//    and pruning mode 0 cull by box alone. t_max = +inf seeds F32_MAX, the walk's "none": no bound,
//    and the answer is "any hit at all" as the closest-hit search defines a hit.
//  * A lane is finished the moment a best drops below the seed; its byte is written and the lane
//    takes the chunk's next ray. No record is built: no trace_end, no hit identity, no uv.
//  * Candidates with a NaN distance (a ray lying exactly in a triangle's plane) are ignored: the
//    walk's nan_hit flag is dropped before phase_end would rerun the sweep for it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
#include "rt_occlusion_walk.h"
#include "rt_path_common.h"
#include "rt_query_frame.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

using namespace rtk;

struct OcclusionArgs {
    const float4* __restrict__ rays;  // rt_occlusion_ray[count]: {origin.xyz, pad}, {direction.xyz, t_max}
    uint8_t* __restrict__ occluded;   // one byte per ray
    ChunkArgs chunks;
};

template <int kMode, bool kTris, uint32_t kThreads>
__global__ void __launch_bounds__(kThreads, 1) rt_occlusion_kernel(KernelArgs ka, OcclusionArgs qa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x;
    SceneView sv = global_scene_view<kMode, kTris>(ka, nullptr);
    // The walk's tables of the LDS image (no record is built: the spheres' materials are left out).
    // Written out here, not through stage_walk_tables / stage_triangle_tables of rt_query_frame.h:
    // with them the (1, triangles) instance has 34 SGPR spills instead of 31.
    if constexpr (kMode >= 1) {
        float4* l_sph = reinterpret_cast<float4*>(lds);
        RtObject* l_obj = reinterpret_cast<RtObject*>(lds + ka.lds_obj_offset);
        uint32_t* l_orig = reinterpret_cast<uint32_t*>(lds + ka.lds_orig_offset);
        float4* l_nodes = reinterpret_cast<float4*>(lds + ka.lds_nodes_offset);
        for (uint32_t i = tid; i < ka.sphere_slot_count; i += kThreads) {
            l_sph[i] = ka.sphere_slots[i];
            l_orig[i] = ka.sphere_orig[i];
        }
        for (uint32_t i = tid; i < 2u * ka.sphere_nodes; i += kThreads) l_nodes[i] = ka.sphere_bvh[i];
        if constexpr (kTris)
            for (uint32_t i = tid; i < ka.object_count; i += kThreads) l_obj[i] = ka.objects[i];
        sv.sph = l_sph;
        sv.orig = l_orig;
        sv.nodes = l_nodes;
        sv.obj = l_obj;
    }
    if constexpr (kMode == 2) {
        float4* l_tn = reinterpret_cast<float4*>(lds + ka.lds_tri_nodes_offset);
        uint4* l_tp = reinterpret_cast<uint4*>(lds + ka.lds_tri_prims_offset);
        for (uint32_t i = tid; i < 2u * ka.tri_nodes; i += kThreads) l_tn[i] = ka.tri_bvh[i];
        for (uint32_t i = tid; i < ka.tri_prim_count; i += kThreads) l_tp[i] = ka.tri_prims[i];
        sv.tri_nodes = l_tn;
        sv.tri_prims = l_tp;
        if (ka.lds_sub_offset) {
            RtSubObject* l_sub = reinterpret_cast<RtSubObject*>(lds + ka.lds_sub_offset);
            for (uint32_t i = tid; i < ka.sub_object_count; i += kThreads) l_sub[i] = ka.sub_objects[i];
            sv.sub = l_sub;
        }
    }
    if constexpr (kMode >= 1) __syncthreads();

    // Lane states. A lane owns one ray at a time.
    constexpr uint32_t kIdle = 0, kSetup = 1, kTrav = 2, kDone = 3;
    uint32_t mode = kIdle;
    unsigned long long ray = 0;
    f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
    float bound = 0.0f;  // the seed: min(t_max, F32_MAX), or 0 for a t_max that nothing is closer than
    TraceState ts = idle_trace_state(0.0f);

    const uint32_t wave = wave_in_launch<kThreads>();
    WaveChunk c{0, 0, true, false};
    claim_chunk(qa.chunks, wave, c);

    while (true) {
        // 1. The bytes of the lanes whose search has finished.
        if (mode == kDone) {
            qa.occluded[ray] = occluder_found(ts, bound) ? (uint8_t)1 : (uint8_t)0;
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
                    // t_max <= 0 or NaN: nothing is closer (the search is skipped)
                    bound = r1.w > 0.0f ? fminf(r1.w, kF32Max) : 0.0f;
                    mode = kSetup;
                }
            }
            c.next += min((uint32_t)__popcll(need), avail);
            if (c.next == c.end) claim_chunk(qa.chunks, wave, c);
        }
        // 3. Start the search of every lane that took a ray.
        if (mode == kSetup) {
            if (bound > 0.0f) {
                occlusion_begin<kTris>(sv, ka, o, d, bound, ts);
                mode = ts.phase == 2 ? kDone : kTrav;
            } else {
                ts.sph.t = ts.tri.t = 0.0f;
                mode = kDone;
            }
        }
        if (__ballot(mode != kIdle) == 0 && c.dry) break;
        // 4. Traverse (query_traverse): finished lanes wait for the wave, which then writes their
        // bytes and refills them together; with no rays left it traverses to the end.
        take_lane_walk(query_traverse<kMode, kTris, false>(sv, ka, o, d, lane_walk(ts, mode), c.dry, lds, OccluderEnd{bound}),
                       ts, mode);
    }
}

// The instances, (mode, triangles, threads): f(kernel, threads) for the one of (mode, tris). The
// workgroup sizes are the closest-hit query's (query.hip).
template <class F>
static hipError_t with_occlusion_instance(int mode, bool tris, F f) {
    if (mode == 0 && tris) return f(&rt_occlusion_kernel<0, true, 256>, 256u);
    if (mode == 1 && tris) return f(&rt_occlusion_kernel<1, true, 1024>, 1024u);
    if (mode == 2 && tris) return f(&rt_occlusion_kernel<2, true, 1024>, 1024u);
    if (mode == 0 && !tris) return f(&rt_occlusion_kernel<0, false, 256>, 256u);
    if (mode == 1 && !tris) return f(&rt_occlusion_kernel<1, false, 1024>, 1024u);
    return hipErrorInvalidValue;
}

// (0 for a (mode, tris) without an instance, as rt_query_threads)
uint32_t rt_occlusion_threads(int mode, bool tris) {
    uint32_t threads = 0;
    (void)with_occlusion_instance(mode, tris, [&](auto, uint32_t t) { return threads = t, hipSuccess; });
    return threads;
}

hipError_t rt_occlusion_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return with_occlusion_instance(
        mode, tris, [&](auto kernel, uint32_t t) { return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu); });
}

hipError_t rt_launch_occlusion(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                               const void* rays, void* occluded, uint64_t count, unsigned long long* counter,
                               hipStream_t stream) {
    if (s.blocks == 0 || count == 0) return hipSuccess;
    return with_occlusion_instance(mode, tris, [&](auto kernel, uint32_t t) {
        const OcclusionArgs qa{static_cast<const float4*>(rays), static_cast<uint8_t*>(occluded),
                               chunk_args(count, counter, s, t)};
        return query_launch_of(kernel, t, s.blocks, lds_bytes, stream, ka, qa);
    });
}
