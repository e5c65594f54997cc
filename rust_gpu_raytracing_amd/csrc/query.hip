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
//    prefix sum over the idle lanes), so a wave does not idle behind one long walk.
//  * A ray is read with two 16-B loads (rt_query_ray, 32 B) and its record written with four 16-B
//    stores (rt_hit, 64 B): a wave's finished lanes write whole 64-B segments.
//  * Scene placement is the path kernel's: mode 0 reads everything from global memory (no staging:
//    what small batches launch), mode 1 stages spheres / objects / the sphere BVH in LDS once per
//    workgroup, mode 2 also the triangle accelerator. Every mode returns the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rt_path_common.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

using namespace rtk;

struct QueryArgs {
    const float4* __restrict__ rays;  // rt_query_ray[count]: {origin.xyz, pad}, {direction.xyz, pad}
    uint4* __restrict__ hits;         // rt_hit[count]
    unsigned long long count;
    unsigned long long* __restrict__ next;  // the chunk counter (zero at launch)
    uint32_t wave_chunk;                    // rays per claim
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

// The wave's next chunk of rays: lane 0 claims, the result is wave-uniform (called by whole waves).
__device__ __forceinline__ void claim_chunk(const QueryArgs& qa, unsigned long long& next, unsigned long long& end,
                                            bool& dry) {
    unsigned long long base = 0;
    if ((threadIdx.x & 63u) == 0) base = atomicAdd(qa.next, (unsigned long long)qa.wave_chunk);
    const uint32_t b_lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
    const uint32_t b_hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    base = ((unsigned long long)b_hi << 32) | b_lo;
    dry = base >= qa.count;
    next = dry ? qa.count : base;
    end = (dry || base + qa.wave_chunk >= qa.count) ? qa.count : base + qa.wave_chunk;
}

}  // namespace

template <int kMode, bool kTris, uint32_t kThreads>
__global__ void __launch_bounds__(kThreads, 1) rt_query_kernel(KernelArgs ka, QueryArgs qa) {
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
    // The part of the path kernel's LDS image the search reads, at the same offsets (materials,
    // their glass constants and the sRGB table are shading's: left out).
    if constexpr (kMode >= 1) {
        float4* l_sph = reinterpret_cast<float4*>(lds);
        RtObject* l_obj = reinterpret_cast<RtObject*>(lds + ka.lds_obj_offset);
        uint32_t* l_orig = reinterpret_cast<uint32_t*>(lds + ka.lds_orig_offset);
        uint32_t* l_smat = reinterpret_cast<uint32_t*>(lds + ka.lds_smat_offset);
        float4* l_nodes = reinterpret_cast<float4*>(lds + ka.lds_nodes_offset);
        for (uint32_t i = tid; i < ka.sphere_slot_count; i += kThreads) {
            l_sph[i] = ka.sphere_slots[i];
            l_orig[i] = ka.sphere_orig[i];
        }
        for (uint32_t i = tid; i < ka.sphere_count; i += kThreads) l_smat[i] = ka.sphere_material[i];
        for (uint32_t i = tid; i < 2u * ka.sphere_nodes; i += kThreads) l_nodes[i] = ka.sphere_bvh[i];
        if constexpr (kTris)
            for (uint32_t i = tid; i < ka.object_count; i += kThreads) l_obj[i] = ka.objects[i];
        sv.sph = l_sph;
        sv.orig = l_orig;
        sv.sph_mat = l_smat;
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
    TraceState ts;
    ts.inv = mk(0.f, 0.f, 0.f);
    ts.a4 = ts.a2 = 0.f;
    ts.node = 0;
    ts.phase = 2;
    ts.pending = kNoLeaf;
    ts.nan_hit = false;
    ts.sph = SphereHit{kF32Max, 0u, 0u};
    ts.tri = TriHit{kF32Max, 0u, 0u, 0u, false};

    // The wave's chunk [next, end) of the ray array, wave-uniform.
    unsigned long long next = 0, end = 0;
    bool dry = false;  // the counter ran past the last ray
    claim_chunk(qa, next, end, dry);

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
                    mode = kSetup;
                }
            }
            next += min((uint32_t)__popcll(need), avail);
            if (next == end) claim_chunk(qa, next, end, dry);
        }
        // 3. Start the search of every lane that took a ray.
        if (mode == kSetup) {
            trace_begin<kTris>(sv, ka, o, d, ts);
            mode = ts.phase == 2 ? kDone : kTrav;
        }
        if (__ballot(mode != kIdle) == 0 && dry) break;
        // 4. Traverse, as the path kernel does (pathtrace.hip, step 4): lanes whose search finishes
        // wait until at most trav_threshold lanes still traverse, then the wave writes their
        // records and refills them together; with no rays left it traverses to the end (a
        // finished ray has no next segment that an earlier return would start sooner).
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
                    if (act) {
                        phase_end<kTris>(sv, ka, o, d, ts);
                        if (ts.phase == 2) mode = kDone;
                    }
                    batched = true;
                }
            }
            if (!batched && mode == kTrav && (!leaves || ts.pending != kNoLeaf)) {
                if (kDeferLeaves<kTris> && leaves) {
                    leaf_step<kTris, (kMode <= 1)>(sv, ka, o, d, ts);
                } else {
                    node_step<kTris, kCertWalk<kMode>>(sv, ka, o, d, ts);
                }
                phase_end<kTris>(sv, ka, o, d, ts);
                if (ts.phase == 2) mode = kDone;
                if (!(kDeferLeaves<kTris> && leaves)) {
#pragma unroll
                    for (int k = 1; k < kTravUnroll<kMode, kTris>; ++k) {
                        if (mode == kTrav) {
                            node_step<kTris, kCertWalk<kMode>>(sv, ka, o, d, ts);
                            phase_end<kTris>(sv, ka, o, d, ts);
                            if (ts.phase == 2) mode = kDone;
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
                        phase_end<kTris>(sv, ka, o, d, ts);
                        if (ts.phase == 2) mode = kDone;
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
                        phase_end<kTris>(sv, ka, o, d, ts);
                        if (ts.phase == 2) mode = kDone;
                    }
                }
            }
        }
    }
}

// Workgroup size by placement: the global-memory instance has no image to share, so small
// workgroups (more of them resident, started sooner); the staged instances share one image among
// 16 waves as the path kernel's largest workgroup does.
uint32_t rt_query_threads(int mode) { return mode == 0 ? 256u : 1024u; }

// (mode, triangles, threads)
#define RT_FOR_EACH_QUERY(X) \
    X(0, true, 256) X(1, true, 1024) X(2, true, 1024) X(0, false, 256) X(1, false, 1024)

// Resident workgroups per CU of the instance at this dynamic LDS size (0: it does not fit).
hipError_t rt_query_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
#define RT_QOCC(M, TR, T)                                                                                   \
    if (mode == M && tris == TR) {                                                                          \
        const void* fn = reinterpret_cast<const void*>(&rt_query_kernel<M, TR, T>);                        \
        if (lds_bytes > 64u * 1024u) {                                                                      \
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); \
            if (e != hipSuccess) return e;                                                                  \
        }                                                                                                   \
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, rt_query_kernel<M, TR, T>, T, lds_bytes); \
    }
    RT_FOR_EACH_QUERY(RT_QOCC)
#undef RT_QOCC
    return hipErrorInvalidValue;
}

hipError_t rt_launch_query(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, uint32_t blocks,
                           const void* rays, void* hits, uint64_t count, unsigned long long* counter,
                           uint32_t wave_chunk, hipStream_t stream) {
    if (blocks == 0 || count == 0) return hipSuccess;
    const QueryArgs qa{static_cast<const float4*>(rays), static_cast<uint4*>(hits), count, counter, wave_chunk};
#define RT_QLAUNCH(M, TR, T)                                                                               \
    if (mode == M && tris == TR) {                                                                         \
        hipLaunchKernelGGL((rt_query_kernel<M, TR, T>), dim3(blocks), dim3(T), lds_bytes, stream, ka, qa); \
        return hipGetLastError();                                                                          \
    }
    RT_FOR_EACH_QUERY(RT_QLAUNCH)
#undef RT_QLAUNCH
    return hipErrorInvalidValue;
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
