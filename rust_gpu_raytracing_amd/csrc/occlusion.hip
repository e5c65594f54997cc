// occlusion.hip -- batched any-hit ray queries for gfx950 (rt_occluded, rt_occluded_device;
// DESIGN.md §5.4c).
//
// rt_occlusion_kernel answers "is anything in the way before t_max?" for arbitrary rays: one byte
// per ray, 1 iff at least one primitive, tested on its own by the reference's test, is accepted at
// a non-NaN distance t < t_max. It stands on the query kernels' frame (rt_query_frame.h): one ray
// per lane, persistent wave64s taking chunks of rays (each wave's own first chunk, then claims from
// one device counter), ballot + mbcnt refill, the three scene placements, the walk of rt_walk.h.
// What differs from the closest-hit query (query.hip):
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

namespace {

// A candidate was accepted: the walk replaces a best only by a strictly closer candidate (the
// seed's tie-break position is 0, which no candidate undercuts), so either best below the seed
// is a primitive accepted at t < bound. Neither is ever NaN (sphere_candidate requires t > 0,
// tri_leaf and coop_leaf_batch route NaN distances to nan_hit).
__device__ __forceinline__ bool occluder_found(const TraceState& ts, float bound) {
    return ts.sph.t < bound || ts.tri.t < bound;
}

// check_triangles (compute_shader.wgsl:422-517) as an any-hit sweep, for scenes whose triangle
// accelerator is off: the first triangle accepted at a non-NaN distance below `bound` decides (the
// sweep's order is free for an any-hit answer). Each test is tri_leaf's.
__device__ __forceinline__ bool sweep_any_triangle(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, f3 inv,
                                                   float bound) {
    const uint32_t n_obj = ka.object_count;
    for (uint32_t oi = 0; oi < n_obj; ++oi) {
        const RtObject& ob = sv.obj[oi];
        if (!ray_in_bounds(o, inv, ob.min_bounds, ob.max_bounds)) continue;
        const uint32_t first_sub = ob.first_sub_object_index;
        const uint32_t n_sub = ob.sub_object_count;
        for (uint32_t i = 0; i < n_sub; ++i) {
            const uint32_t si = min(first_sub + i, ka.sub_object_count - 1u);
            const RtSubObject sub = sv.sub[si];
            if (!ray_in_bounds(o, inv, sub.min_bounds, sub.max_bounds)) continue;
            for (uint32_t j = 0; j < sub.triangle_count; ++j) {
                const uint32_t ti = min(sub.first_triangle_index + j, ka.triangle_count - 1u);
                const TriGeom g = load_tri(ka.triangles, ti);
                const float det = -dot(d, g.cn);
                const float inv_det = 1.0f / det;
                const f3 ao = o - g.a;
                const float dist = dot(ao, g.cn) * inv_det;
                if (!(dist < bound) || dist < 0.0f) continue;  // (a NaN distance never occludes)
                const f3 dao = cross(ao, d);
                const float v = -dot(g.ab, dao) * inv_det;
                if (v < 0.0f) continue;
                const float u = dot(g.ac, dao) * inv_det;
                if (u < 0.0f) continue;
                const float w = 1.0f - u - v;
                if (w < 0.0f) continue;
                return true;
            }
        }
    }
    return false;
}

// trace_begin (rt_walk.h) for an any-hit search bounded by `bound` in (0, F32_MAX]: the bests are
// seeded with the bound, and the search is over (ts.phase == 2) as soon as the brute-force sphere
// set or the sweep finds an occluder.
template <bool kTris>
__device__ __forceinline__ void occlusion_begin(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, float bound,
                                                TraceState& ts) {
    if constexpr (kTris) {
        ts.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);  // ray_in_bounds (:407-419) needs the IEEE quotient
    } else {
        ts.inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    }
    const float a = dot(d, d);
    ts.a4 = 4.0f * a;
    ts.a2 = 2.0f * a;
    ts.sph = SphereHit{bound, 0u, 0u};
    ts.tri = TriHit{bound, 0u, 0u, 0u, false};
    ts.nan_hit = false;
    ts.node = 0;
    ts.pending = kNoLeaf;
    ts.phase = 2;
    // brute-force sphere set, as trace_begin sweeps it
    uint32_t i = 0;
    for (; i + 4u <= ka.sphere_always; i += 4u) test_sphere_group<true>(sv, i, o, d, ts.a4, ts.a2, ts.sph);
    if (ka.sphere_always - i >= 2u) {
        test_sphere_group<true>(sv, i, o, d, ts.a4, ts.a2, ts.sph);
    } else if (ka.sphere_always - i == 1u) {
        float b;
        const float disc = sphere_disc(sv.sph[i], o, d, ts.a4, b);
        sphere_candidate(disc, b, ts.a2, sv.orig[i], i, ts.sph);
    }
    if (occluder_found(ts, bound)) return;
    uint32_t phase;
    if constexpr (!kTris) {
        phase = 1;
    } else if (!ka.tri_accel) {
        if (sweep_any_triangle(sv, ka, o, d, ts.inv, bound)) {
            ts.tri.t = 0.0f;  // below every bound
            return;
        }
        phase = 1;
    } else {
        phase = ka.tri_nodes != 0 ? 0u : 1u;
    }
    if (phase == 1 && ka.sphere_nodes == 0) return;
    ts.phase = phase;
    phase_setup<kTris>(sv, ka, o, a, phase, ts);
}

// What ends a step of the any-hit search: a lane's search ends when its walks do or when an
// occluder is found, whichever is first. (NaN candidates never occlude: the flag is dropped so
// that phase_end does not sweep for it.)
struct OccluderEnd {
    float bound;
    template <bool kTris>
    __device__ __forceinline__ void step(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts,
                                         uint32_t& mode) const {
        ts.nan_hit = false;
        phase_end<kTris>(sv, ka, o, d, ts);
        if (ts.phase == 2 || occluder_found(ts, bound)) mode = kLaneDone;
    }
};

}  // namespace

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
