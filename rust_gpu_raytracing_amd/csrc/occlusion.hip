// occlusion.hip -- batched any-hit ray queries for gfx950 (rt_occluded, rt_occluded_device;
// DESIGN.md §5.4c).
//
// rt_occlusion_kernel answers "is anything in the way before t_max?" for arbitrary rays: one byte
// per ray, 1 iff at least one primitive, tested on its own by the reference's test, is accepted at
// a non-NaN distance t < t_max. It stands on rt_query_kernel's frame (query.hip): one ray per lane,
// persistent wave64s claiming chunks of rays from one device counter, ballot + mbcnt refill, the
// three scene placements, the walk of rt_walk.h. What differs:
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
#include "rt_walk.h"

#pragma clang fp contract(off)

using namespace rtk;

struct OcclusionArgs {
    const float4* __restrict__ rays;  // rt_occlusion_ray[count]: {origin.xyz, pad}, {direction.xyz, t_max}
    uint8_t* __restrict__ occluded;   // one byte per ray
    unsigned long long count;
    unsigned long long* __restrict__ next;  // the chunk counter (zero at launch)
    uint32_t wave_chunk;                    // rays per claim
    uint32_t first_chunk;                   // rays of each wave's own first chunk (no claim)
    unsigned long long claimed_from;        // first ray handed out by the counter: first_chunk x the launch's waves
};

namespace {

// The wave's next chunk of rays, wave-uniform (called by whole waves). The first chunk is the
// wave's own, by its index in the launch: were it claimed, every resident wave's first claim would
// queue at one counter address while nothing else runs. After it lane 0 claims from the counter,
// which hands out the rays from qa.claimed_from on; a launch whose first chunks cover every ray
// claims nothing. (Reading the counter before claiming, to spare the claim that comes back empty,
// doubled the run time of 2M rays: a load of that line queues with the claims. DESIGN.md §5.4c.)
__device__ __forceinline__ void claim_chunk(const OcclusionArgs& qa, uint32_t wave, bool& first,
                                            unsigned long long& next, unsigned long long& end, bool& dry) {
    unsigned long long base = qa.count, chunk = qa.wave_chunk;
    if (first) {
        base = (unsigned long long)wave * qa.first_chunk;
        chunk = qa.first_chunk;
        first = false;
    }
    if (base >= qa.count && qa.claimed_from < qa.count) {
        unsigned long long got = qa.count;
        if ((threadIdx.x & 63u) == 0) got = atomicAdd(qa.next, (unsigned long long)qa.wave_chunk);
        const uint32_t b_lo = __builtin_amdgcn_readfirstlane((uint32_t)got);
        const uint32_t b_hi = __builtin_amdgcn_readfirstlane((uint32_t)(got >> 32));
        base = qa.claimed_from + (((unsigned long long)b_hi << 32) | b_lo);
        chunk = qa.wave_chunk;
    }
    dry = base >= qa.count;
    next = dry ? qa.count : base;
    end = (dry || base + chunk >= qa.count) ? qa.count : base + chunk;
}

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

}  // namespace

template <int kMode, bool kTris, uint32_t kThreads>
__global__ void __launch_bounds__(kThreads, 1) rt_occlusion_kernel(KernelArgs ka, OcclusionArgs qa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x;
    SceneView sv{ka.sphere_slots, ka.sphere_orig, ka.sphere_material, ka.sphere_bvh, ka.materials, nullptr,
                 ka.objects,      nullptr,        ka.tri_bvh,         ka.tri_prims,  kTris ? *ka.tri_extent : 0.0f,
                 ka.sub_objects};
    if constexpr (kTris && kMode <= 1) {
        if (ka.tri_qnodes) {
            const float4 g0 = ka.tri_qgrid[0], g1 = ka.tri_qgrid[1];
            if (g0.w != 0.0f) {
                sv.tri_q = ka.tri_qnodes;
                sv.qox = g0.x;
                sv.qoy = g0.y;
                sv.qoz = g0.z;
                sv.qsx = g1.x;
                sv.qsy = g1.y;
                sv.qsz = g1.z;
            }
        }
    }
    // The LDS image of the placement, as rt_query_kernel stages it (the same offsets).
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
    TraceState ts;
    ts.inv = mk(0.f, 0.f, 0.f);
    ts.a4 = ts.a2 = 0.f;
    ts.node = 0;
    ts.phase = 2;
    ts.pending = kNoLeaf;
    ts.nan_hit = false;
    ts.sph = SphereHit{0.0f, 0u, 0u};
    ts.tri = TriHit{0.0f, 0u, 0u, 0u, false};

    // A lane's search ends when its walks do or when an occluder is found, whichever is first.
    // (NaN candidates never occlude: the flag is dropped so that phase_end does not sweep for it.)
    auto step_end = [&]() {
        ts.nan_hit = false;
        phase_end<kTris>(sv, ka, o, d, ts);
        if (ts.phase == 2 || occluder_found(ts, bound)) mode = kDone;
    };

    // The wave's chunk [next, end) of the ray array, wave-uniform.
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64u) + (tid >> 6));
    bool first = true;
    unsigned long long next = 0, end = 0;
    bool dry = false;  // no rays are left for this wave
    claim_chunk(qa, wave, first, next, end, dry);

    while (true) {
        // 1. The bytes of the lanes whose search has finished.
        if (mode == kDone) {
            qa.occluded[ray] = occluder_found(ts, bound) ? (uint8_t)1 : (uint8_t)0;
            mode = kIdle;
        }
        // 2. Refill: idle lanes take the chunk's next rays, in order.
        while (true) {
            const uint64_t need = __ballot(mode == kIdle);
            if (need == 0 || dry) break;
            const uint32_t avail = (uint32_t)(end - next);
            if (mode == kIdle) {
                const uint32_t rank =
                    __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                if (rank < avail) {
                    ray = next + rank;
                    const float4 r0 = qa.rays[2ull * ray], r1 = qa.rays[2ull * ray + 1ull];
                    o = mk(r0.x, r0.y, r0.z);
                    d = mk(r1.x, r1.y, r1.z);
                    // t_max <= 0 or NaN: nothing is closer (the search is skipped)
                    bound = r1.w > 0.0f ? fminf(r1.w, kF32Max) : 0.0f;
                    mode = kSetup;
                }
            }
            next += min((uint32_t)__popcll(need), avail);
            if (next == end) claim_chunk(qa, wave, first, next, end, dry);
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
        if (__ballot(mode != kIdle) == 0 && dry) break;
        // 4. Traverse, as rt_query_kernel does: lanes whose search finishes wait until at most
        // trav_threshold lanes still traverse, then the wave writes their bytes and refills them
        // together; with no rays left it traverses to the end.
        const uint32_t thresh = dry ? 0u : ka.trav_threshold;
        while (true) {
            const uint64_t trav = __ballot(mode == kTrav);
            const uint32_t n_trav = (uint32_t)__popcll(trav);
            if (n_trav <= thresh || trav == 0) break;
            bool leaves = false;
            if constexpr (kDeferLeaves<kTris> && !kFusedLeaves<kMode, kTris>) {
                const uint32_t n_pend = (uint32_t)__popcll(__ballot(mode == kTrav && ts.pending != kNoLeaf));
                leaves = 8u * n_pend >= ka.leaf_batch * n_trav;
            }
            bool batched = false;
            if constexpr (kCoopLeaves<kMode, kTris>) {
                if (leaves && ka.tri_leaftris) {  // the wave's deferred leaves, cooperatively
                    const bool act = mode == kTrav && ts.pending != kNoLeaf;
                    coop_leaf_batch(sv, ka, o, d, ts, act, lds);
                    if (act) step_end();
                    batched = true;
                }
            }
            if (!batched && mode == kTrav && (!leaves || ts.pending != kNoLeaf)) {
                if (kDeferLeaves<kTris> && leaves) {
                    leaf_step<kTris, (kMode <= 1)>(sv, ka, o, d, ts);
                } else {
                    node_step<kTris, kCertWalk<kMode>>(sv, ka, o, d, ts);
                }
                step_end();
                if (!(kDeferLeaves<kTris> && leaves)) {
#pragma unroll
                    for (int k = 1; k < kTravUnroll<kMode, kTris>; ++k) {
                        if (mode == kTrav) {
                            node_step<kTris, kCertWalk<kMode>>(sv, ka, o, d, ts);
                            step_end();
                        }
                    }
                }
                if constexpr (kFusedLeaves<kMode, kTris>) {
                    // the leaf batch after the block's node steps: one kind of leaf per batch
                    const uint64_t mt = __ballot(mode == kTrav && ts.pending != kNoLeaf && ts.phase == 0);
                    const uint64_t ms = __ballot(mode == kTrav && ts.pending != kNoLeaf && ts.phase != 0);
                    const uint32_t n_p = (uint32_t)__popcll(mt | ms);
                    const uint32_t n_t = (uint32_t)__popcll(__ballot(mode == kTrav));
                    const bool tri_first = __popcll(mt) >= __popcll(ms);
                    if (8u * n_p >= ka.leaf_batch * n_t && mode == kTrav && ts.pending != kNoLeaf &&
                        (ts.phase == 0) == tri_first) {
                        leaf_step<kTris, (kMode <= 1)>(sv, ka, o, d, ts);
                        step_end();
                    }
                }
                if constexpr (kBlockLeaves<kTris>) {
                    // the block's group tests: every lane that reached a leaf in it, together
                    const uint32_t n_wait = (uint32_t)__popcll(__ballot(ts.pending != kNoLeaf));
                    const uint32_t n_tr = (uint32_t)__popcll(__ballot(true));
                    if (8u * n_wait >= kBlockLeafShare * n_tr && mode == kTrav && ts.pending != kNoLeaf) {
                        test_sphere_group(sv, ts.pending, o, d, ts.a4, ts.a2, ts.sph);
                        ts.limit = prune_limit(ts);
                        ts.pending = kNoLeaf;
                        step_end();
                    }
                }
            }
        }
    }
}

// Workgroup size by placement, as the closest-hit query's (query.hip).
uint32_t rt_occlusion_threads(int mode) { return mode == 0 ? 256u : 1024u; }

// (mode, triangles, threads)
#define RT_FOR_EACH_OCCLUSION(X) \
    X(0, true, 256) X(1, true, 1024) X(2, true, 1024) X(0, false, 256) X(1, false, 1024)

// Resident workgroups per CU of the instance at this dynamic LDS size (0: it does not fit).
hipError_t rt_occlusion_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
#define RT_OOCC(M, TR, T)                                                                                \
    if (mode == M && tris == TR) {                                                                          \
        const void* fn = reinterpret_cast<const void*>(&rt_occlusion_kernel<M, TR, T>);                  \
        if (lds_bytes > 64u * 1024u) {                                                                      \
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); \
            if (e != hipSuccess) return e;                                                                  \
        }                                                                                                   \
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, rt_occlusion_kernel<M, TR, T>, T, \
                                                            lds_bytes);                                    \
    }
    RT_FOR_EACH_OCCLUSION(RT_OOCC)
#undef RT_OOCC
    return hipErrorInvalidValue;
}

hipError_t rt_launch_occlusion(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, uint32_t blocks,
                               const void* rays, void* occluded, uint64_t count, unsigned long long* counter,
                               uint32_t wave_chunk, uint32_t first_chunk, hipStream_t stream) {
    if (blocks == 0 || count == 0) return hipSuccess;
    const unsigned long long waves = (unsigned long long)blocks * (rt_occlusion_threads(mode) / 64u);
    const OcclusionArgs qa{static_cast<const float4*>(rays), static_cast<uint8_t*>(occluded), count, counter,
                           wave_chunk, first_chunk, waves * first_chunk};
#define RT_OLAUNCH(M, TR, T)                                                                                  \
    if (mode == M && tris == TR) {                                                                               \
        hipLaunchKernelGGL((rt_occlusion_kernel<M, TR, T>), dim3(blocks), dim3(T), lds_bytes, stream, ka, qa); \
        return hipGetLastError();                                                                                \
    }
    RT_FOR_EACH_OCCLUSION(RT_OLAUNCH)
#undef RT_OLAUNCH
    return hipErrorInvalidValue;
}
