// hits.hip -- batched hit-list ray queries for gfx950 (rt_trace_hits, rt_trace_hits_device,
// rt_pick_hits).
//
// rt_hits_kernel answers "what are the things along this ray, in order?" for arbitrary rays: the
// max_hits nearest primitives of each ray as rt_hit records. The contract (include/rt_abi.h):
//
// THE HIT-LIST CONTRACT. For the ray (o, d, t_max) and a list length max_hits in 1..RT_HITS_MAX:
//  1. Bound. bound = min(t_max, 3.4028235e38f). A t_max that is <= 0 or NaN gives no candidates.
//  2. Sphere candidates. Sphere i is a candidate when the test of check_spheres
//     (compute_shader.wgsl:355-404) on it alone accepts it: not disc < 0, and
//     t = (-b - sqrt(disc)) / (2a) with t > 0; and t < bound. One candidate per sphere, the near
//     root, as in the reference.
//  3. Triangle candidates. A visit (object oi, sub-object slot i, triangle slot j) of the sweep of
//     check_triangles (:422-517) is a candidate when it is behind the ray_in_bounds tests of its
//     object and of its sub-object, with the reference's index clamps; none of the reference's
//     rejections dist < 0, v < 0, u < 0, w < 0 holds (dist >= 0 and u, v, w >= 0); and its
//     distance is not NaN and is < bound. Its sweep position seq is its position in the sweep's
//     order over all (object, sub-object slot, triangle slot) triples, boxes disregarded.
//  4. NaN distances. A candidate with a NaN distance is never listed: the any-hit rule, and the
//     one difference from the closest-hit record.
//  5. Order. Ascending t. At equal t triangles come before spheres, triangles ascend by seq and
//     spheres ascend by index as uploaded: the order in which trace_ray (:342-353) and the two
//     sweeps would prefer them.
//  6. Result. n = min(number of candidates, max_hits). Entries 0..n-1 are the first n candidates
//     in that order, each the rt_hit record rt_trace_rays builds for that primitive at that t:
//     position, facing normal, u and v whatever the texture size, material, front_face, kind,
//     index, sub_object, triangle. Entries n..max_hits-1 are the miss record: all zero,
//     t = 3.4028235e38f. counts[i] = n. Every entry of every ray is written and nothing else is.
//
// The kernel stands on the query kernels' frame (rt_query_frame.h): one ray per lane, persistent
// wave64s claiming chunks of rays from one device counter, ballot + mbcnt refill, the three scene
// placements staged as query.hip stages them. What is its own:
//
//  * The lane's list lives in the ray's own records. Entry j of the list being built is the first
//    16 bytes of record j of that ray: {t, order key, two words of identity}, kept sorted by
//    insertion. No register array, no LDS slab: the same code serves every max_hits and every
//    placement at the registers of a one-entry search. Only the count and the bound stay in
//    registers. When the walks end the entries are expanded in place, first to last, into the
//    64-byte records (an entry is read before its record is written over it).
//  * The order key is one word: a triangle's sweep position, or 2^31 + a sphere's index as
//    uploaded. (t, key) ascending is the contract's order, and keys are unique.
//  * The bound. While the list is not full the bound is the ray's (bound, key 0: only a strictly
//    smaller t precedes it); once full it is the last entry's (t, key). A candidate is accepted
//    when (t, key) precedes the bound, so a candidate at exactly the last entry's t with a lower
//    key is still taken. Both running bests of the TraceState are kept at the bound's t: the
//    sphere walk's prune_limit, whose slack is proved for "cannot be accepted at a distance <= b"
//    (a closest-hit search must find ties too), then culls for the list as it culls for a best
//    hit. The triangle walk culls by box, which is exact without any bound, and on the walks from
//    global memory by the leaf certificates of §5.3c (tri_leaf_skips), which prove "cannot be
//    accepted at a distance <= tb": a leaf entered beyond the bound's t is tested against its
//    certificate with tb = that t, so a tie at exactly the bound is still visited.
//  * Leaves report every accepted primitive: a leaf inserts each candidate on its own where
//    tri_leaf and test_sphere_group keep a leaf's minimum. Leaves are tested where the walk
//    reaches them (no deferred or cooperative batches).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
#include "rt_path_common.h"
#include "rt_query_frame.h"
#include "rt_walk.h"

#pragma clang fp contract(off)

using namespace rtk;

struct HitsArgs {
    const float4* __restrict__ rays;  // rt_occlusion_ray[count]: {origin.xyz, pad}, {direction.xyz, t_max}
    uint4* hits;                      // rt_hit[count * max_hits]; a ray's list is built in its own records
    uint32_t* counts;                 // one per ray, or null
    uint32_t max_hits;                // 1..RT_HITS_MAX
    uint32_t pick;                    // 1: the rays carry no t_max (rt_pick_hits' ray): +inf
    ChunkArgs chunks;                 // every chunk is claimed: first_chunk and claimed_from are 0
};

namespace {

constexpr uint32_t kSphereKey = 0x80000000u;  // order key of sphere i: kSphereKey + i (after every triangle)

// A lane's list: `n` entries of {t, key, a, b} at e[0], e[4], ... (the first 16 bytes of the ray's
// records), ascending by (t, key). (bt, bkey): what a candidate must precede to be accepted.
struct LaneList {
    uint4* e;
    uint32_t n;
    float bt;
    uint32_t bkey;
};

__device__ __forceinline__ bool precedes(float t, uint32_t key, float bt, uint32_t bkey) {
    return t < bt || (t == bt && key < bkey);
}

// Inserts an accepted candidate; of a full list the last entry drops out. The search state's bests
// follow the bound.
__device__ __forceinline__ void list_insert(LaneList& l, uint32_t max_hits, TraceState& ts, float t, uint32_t key,
                                            uint32_t a, uint32_t b) {
    uint32_t j = l.n < max_hits ? l.n : max_hits - 1u;  // the slot that opens: a new last one, or the dropped entry's
    l.n = l.n < max_hits ? l.n + 1u : max_hits;
    while (j > 0u) {
        const uint4 p = l.e[4u * (j - 1u)];
        if (precedes(__uint_as_float(p.x), p.y, t, key)) break;
        l.e[4u * j] = p;
        --j;
    }
    l.e[4u * j] = make_uint4(__float_as_uint(t), key, a, b);
    if (l.n == max_hits) {
        const uint4 last = l.e[4u * (max_hits - 1u)];
        l.bt = __uint_as_float(last.x);
        l.bkey = last.y;
        ts.sph.t = ts.tri.t = l.bt;
    }
}

// check_spheres' test (:372-391) on the sphere of one slot, alone: sphere_disc and
// sphere_candidate's root, accepted against the list's bound instead of a best hit.
__device__ __forceinline__ void list_sphere(const SceneView& sv, uint32_t slot, f3 o, f3 d, TraceState& ts, LaneList& l,
                                            uint32_t max_hits) {
    float b;
    const float disc = sphere_disc(sv.sph[slot], o, d, ts.a4, b);
    if (disc >= 0.0f) {
        const float t = (-b - sphere_root_sqrt(disc)) / ts.a2;
        const uint32_t key = kSphereKey + sv.orig[slot];
        if (t > 0.0f && precedes(t, key, l.bt, l.bkey)) list_insert(l, max_hits, ts, t, key, slot, 0u);
    }
}

// The reference's triangle test (:449-481) on triangle `ti` alone, tri_leaf's operations, accepted
// against the list's bound. A NaN distance is never listed.
__device__ __forceinline__ void list_triangle(const KernelArgs& ka, uint32_t ti, uint32_t seq, uint32_t obj, f3 o, f3 d,
                                              TraceState& ts, LaneList& l, uint32_t max_hits) {
    const TriGeom g = load_tri(ka.triangles, ti);
    const float det = -dot(d, g.cn);
    const float inv_det = 1.0f / det;
    const f3 ao = o - g.a;
    const float dist = dot(ao, g.cn) * inv_det;
    if (dist < 0.0f || !precedes(dist, seq, l.bt, l.bkey)) return;  // (a NaN distance precedes nothing)
    const f3 dao = cross(ao, d);
    const float v = -dot(g.ab, dao) * inv_det;
    if (v < 0.0f) return;
    const float u = dot(g.ac, dao) * inv_det;
    if (u < 0.0f) return;
    const float w = 1.0f - u - v;
    if (w < 0.0f) return;
    list_insert(l, max_hits, ts, dist, seq, ti | (det > 0.0f ? 0x80000000u : 0u), obj);
}

// The triangle leaf (tri_leaf without the minimum): the reference's object and sub-object
// ray_in_bounds tests (:431, :441), then every triangle of the (object, sub-object) pair on its own.
// `skip`: the triangles the leaf's certificate proves unacceptable at a distance <= the bound
// (tri_leaf_skips; they are not loaded).
__device__ __forceinline__ void list_tri_leaf(const SceneView& sv, const KernelArgs& ka, uint32_t prim, uint32_t skip,
                                              f3 o, f3 d, TraceState& ts, LaneList& l, uint32_t max_hits) {
    const uint4 pr = sv.tri_prims[prim];  // object, sub, seq_base, range
    const RtObject& ob = sv.obj[pr.x];
    if (!ray_in_bounds(o, ts.inv, ob.min_bounds, ob.max_bounds)) return;
    const RtSubObject sub = sv.sub[pr.y];
    if (!ray_in_bounds(o, ts.inv, sub.min_bounds, sub.max_bounds)) return;
    for (uint32_t j = 0; j < sub.triangle_count; ++j) {
        if (j < kLeafCertSlots && ((skip >> j) & 1u)) continue;
        list_triangle(ka, min(sub.first_triangle_index + j, ka.triangle_count - 1u), pr.z + j, pr.x, o, d, ts, l,
                      max_hits);
    }
}

// check_triangles (:422-517) for scenes whose triangle accelerator is off: the reference's sweep,
// every visit on its own. seq counts every (object, sub-object slot, triangle slot) triple, behind
// a failed box test too (the accelerator's seq_base, sphere_bvh.cpp).
__device__ __forceinline__ void list_sweep_triangles(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d,
                                                     TraceState& ts, LaneList& l, uint32_t max_hits) {
    uint32_t seq = 0u;
    const uint32_t n_obj = ka.object_count;
    for (uint32_t oi = 0; oi < n_obj; ++oi) {
        const RtObject& ob = sv.obj[oi];
        const bool in_obj = ray_in_bounds(o, ts.inv, ob.min_bounds, ob.max_bounds);
        const uint32_t first_sub = ob.first_sub_object_index;
        const uint32_t n_sub = ob.sub_object_count;
        for (uint32_t i = 0; i < n_sub; ++i) {
            const uint32_t si = min(first_sub + i, ka.sub_object_count - 1u);
            const RtSubObject sub = sv.sub[si];
            if (in_obj && ray_in_bounds(o, ts.inv, sub.min_bounds, sub.max_bounds))
                for (uint32_t j = 0; j < sub.triangle_count; ++j)
                    list_triangle(ka, min(sub.first_triangle_index + j, ka.triangle_count - 1u), seq + j, oi, o, d, ts,
                                  l, max_hits);
            seq += sub.triangle_count;
        }
    }
}

// trace_begin (rt_walk.h) for a list search bounded by l.bt in (0, F32_MAX]: the bests are seeded
// with the bound, the always-tested spheres and (accelerator off) the sweep report every
// candidate, and the first walk is set up. ts.phase == 2: nothing is left to walk.
template <bool kTris>
__device__ __forceinline__ void hits_begin(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts,
                                           LaneList& l, uint32_t max_hits) {
    // ray_in_bounds (:407-419) needs the IEEE quotient; the sphere-only slab test takes v_rcp_f32 (trace_begin)
    if constexpr (kTris) {
        ts.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    } else {
        ts.inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    }
    const float a = dot(d, d);
    ts.a4 = 4.0f * a;
    ts.a2 = 2.0f * a;
    ts.sph = SphereHit{l.bt, 0u, 0u};
    ts.tri = TriHit{l.bt, 0u, 0u, 0u, false};
    ts.nan_hit = false;
    ts.node = 0;
    ts.pending = kNoLeaf;
    for (uint32_t i = 0; i < ka.sphere_always; ++i) list_sphere(sv, i, o, d, ts, l, max_hits);
    if constexpr (!kTris) {
        ts.phase = 1;
    } else if (!ka.tri_accel) {
        list_sweep_triangles(sv, ka, o, d, ts, l, max_hits);
        ts.phase = 1;
    } else {
        ts.phase = ka.tri_nodes != 0 ? 0u : 1u;
    }
    if (ts.phase == 1 && ka.sphere_nodes == 0) ts.phase = 2;
    phase_setup<kTris>(sv, ka, o, a, ts.phase, ts);
}

// One node of the current walk (node_step and node_visit of rt_walk.h with the leaf tested on the
// spot), then phase_end's rule: the triangle walk hands over to the sphere walk, whose end is the
// search's. Skip links only advance, so the walk terminates on any input.
// kCert: the walk reads leaf certificates when ka.tri_leafcert is set (the walks from global
// memory, kCertWalk): a leaf whose box is entered beyond the bound's t is tested against its
// certificate on the spot, as the primary pre-pass tests it, with the bound for the best hit.
template <bool kTris, bool kCert>
__device__ __forceinline__ void hits_step(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, TraceState& ts,
                                          LaneList& l, uint32_t max_hits) {
    const bool tri = kTris && ts.phase == 0;
    float4 lo, hi;
    if (kTris && tri && sv.tri_q) {
        qnode_decode(sv, sv.tri_q[ts.node], ts.node, lo, hi);
    } else {
        const float4* nodes = tri ? sv.tri_nodes : sv.nodes;
        lo = nodes[2u * ts.node];
        hi = nodes[2u * ts.node + 1u];
    }
    float near_t, far_t;
    if (!kTris && ka.sphere_boxes_ordered)
        slab_hit_ordered(ts.slab, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    else
        slab_hit(ts.slab, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, near_t, far_t);
    // node_visit's test: ts.slack / ts.limit are 0 / inf on the triangle side
    const bool hit = near_t <= far_t && far_t >= -ts.slack && near_t <= ts.limit;
    const uint32_t leaf = __float_as_uint(hi.w);
    const bool at_leaf = hit && leaf != 0xffffffffu;
    if (at_leaf) {
        if (tri) {
            uint32_t skip = 0u;
            if constexpr (kCert)
                if (ka.tri_leafcert && near_t > l.bt && l.bt != kF32Max)
                    skip = tri_leaf_skips(ka, leaf & 0xffffffu, ts.slab, o, d, l.bt, lo, hi);
            if (skip != kLeafCertAll) list_tri_leaf(sv, ka, leaf & 0xffffffu, skip, o, d, ts, l, max_hits);
        } else {
            const uint32_t slot = leaf & 0xffffffu;  // an aligned group of 4 slots, padded with NaN spheres
            for (uint32_t k = 0; k < 4u; ++k) list_sphere(sv, slot + k, o, d, ts, l, max_hits);
            ts.limit = prune_limit(ts);
        }
    }
    ts.node = (hit && !at_leaf) ? ts.node + 1u : __float_as_uint(lo.w);
    if (tri) {
        if (ts.node < ka.tri_nodes) return;
        ts.node = 0;
        ts.phase = ka.sphere_nodes != 0 ? 1u : 2u;
        phase_setup<kTris>(sv, ka, o, ts.a2 * 0.5f, 1, ts);
    } else if (ts.node >= ka.sphere_nodes) {
        ts.phase = 2;
    }
}

// The sub-object of object `obj` that holds triangle `tri`, as rt_query_kernel finds it for its
// record (query.hip: a binary search over the object's ascending triangle ranges, else the first
// record in order that holds the triangle).
__device__ __forceinline__ uint32_t hits_sub_object(const SceneView& sv, const KernelArgs& ka, uint32_t obj,
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

// The 64-byte record of one list entry, as rt_query_kernel writes the record of that primitive at
// that t: the search state trace_end reads is set to the entry alone.
template <bool kTris>
__device__ __forceinline__ void write_entry(const SceneView& sv, const KernelArgs& ka, f3 o, f3 d, uint4 e, uint4* rec) {
    TraceState ts;
    ts.sph = SphereHit{kF32Max, 0u, 0u};
    ts.tri = TriHit{kF32Max, 0u, 0u, 0u, false};
    if (e.y >= kSphereKey)
        ts.sph = SphereHit{__uint_as_float(e.x), e.y - kSphereKey, e.z};
    else
        ts.tri = TriHit{__uint_as_float(e.x), e.y, e.z & 0x7fffffffu, e.w, (e.z >> 31) != 0u};
    const Hit h = trace_end<kTris, true>(sv, ka, o, d, ts);
    const HitId id = trace_end_id<kTris>(ts);
    uint32_t sub = 0u;
    if constexpr (kTris)
        if (id.kind == 2u) sub = hits_sub_object(sv, ka, id.index, id.triangle);
    rec[0] = make_uint4(__float_as_uint(h.t), __float_as_uint(h.p.x), __float_as_uint(h.p.y), __float_as_uint(h.p.z));
    rec[1] = make_uint4(__float_as_uint(h.n.x), __float_as_uint(h.n.y), __float_as_uint(h.n.z), __float_as_uint(h.u));
    rec[2] = make_uint4(__float_as_uint(h.v), h.material_index, h.front_face ? 1u : 0u, id.kind);
    rec[3] = make_uint4(id.index, sub, id.triangle, 0u);
}

}  // namespace

template <int kMode, bool kTris, uint32_t kThreads>
__global__ void __launch_bounds__(kThreads, 1) rt_hits_kernel(KernelArgs ka, HitsArgs qa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // The closest-hit query's image (query.hip): what the search and the record read.
    SceneView sv = global_scene_view<kMode, kTris>(ka, nullptr);
    if constexpr (kMode >= 1) {
        sv = stage_walk_tables<kTris, kThreads>(ka, lds, sv);
        sv = stage_sphere_materials<kThreads>(ka, lds, sv);
    }
    if constexpr (kMode == 2) sv = stage_triangle_tables<kThreads>(ka, lds, sv);
    if constexpr (kMode >= 1) __syncthreads();

    // Lane states. A lane owns one ray at a time.
    constexpr uint32_t kIdle = 0, kSetup = 1, kTrav = 2, kDone = 3;
    const uint32_t max_hits = qa.max_hits;
    uint32_t mode = kIdle;
    unsigned long long ray = 0;
    f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
    TraceState ts = idle_trace_state(0.0f);
    LaneList l{qa.hits, 0u, 0.0f, 0u};

    // Every chunk comes from the counter, as in the closest-hit kernel.
    WaveChunk c{0, 0, false, false};
    claim_chunk<false>(qa.chunks, 0u, c);

    while (true) {
        // 1. The records of the lanes whose search has finished: the listed entries first to last
        // (each read before its record takes its place), then the miss records, then the count.
        if (mode == kDone) {
            for (uint32_t j = 0; j < l.n; ++j) write_entry<kTris>(sv, ka, o, d, l.e[4u * j], l.e + 4u * j);
            for (uint32_t j = l.n; j < max_hits; ++j) {
                uint4* rec = l.e + 4u * j;
                rec[0] = make_uint4(__float_as_uint(kF32Max), 0u, 0u, 0u);
                rec[1] = rec[2] = rec[3] = make_uint4(0u, 0u, 0u, 0u);
            }
            if (qa.counts) qa.counts[ray] = l.n;
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
                    const float t_max = qa.pick ? __builtin_inff() : r1.w;
                    // t_max <= 0 or NaN: no candidates (the search is skipped)
                    l = LaneList{qa.hits + 4ull * max_hits * ray, 0u, t_max > 0.0f ? fminf(t_max, kF32Max) : 0.0f, 0u};
                    mode = kSetup;
                }
            }
            c.next += min((uint32_t)__popcll(need), avail);
            if (c.next == c.end) claim_chunk<false>(qa.chunks, 0u, c);
        }
        // 3. Start the search of every lane that took a ray.
        if (mode == kSetup) {
            mode = kDone;
            if (l.bt > 0.0f) {
                hits_begin<kTris>(sv, ka, o, d, ts, l, max_hits);
                if (ts.phase != 2) mode = kTrav;
            }
        }
        if (__ballot(mode != kIdle) == 0 && c.dry) break;
        // 4. Traverse in blocks of node steps until at most trav_threshold lanes still do (finished
        // lanes are then written and refilled together), or to the end once no rays are left.
        const uint32_t thresh = c.dry ? 0u : ka.trav_threshold;
        while (true) {
            const uint32_t n_trav = (uint32_t)__popcll(__ballot(mode == kTrav));
            if (n_trav <= thresh || n_trav == 0u) break;
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                if (mode == kTrav) {
                    hits_step<kTris, kCertWalk<kMode>>(sv, ka, o, d, ts, l, max_hits);
                    if (ts.phase == 2) mode = kDone;
                }
            }
        }
    }
}

// The instances, (mode, triangles, threads): f(kernel, threads) for the one of (mode, tris). The
// workgroup sizes are the closest-hit query's (query.hip).
template <class F>
static hipError_t with_hits_instance(int mode, bool tris, F f) {
    if (mode == 0 && tris) return f(&rt_hits_kernel<0, true, 256>, 256u);
    if (mode == 1 && tris) return f(&rt_hits_kernel<1, true, 1024>, 1024u);
    if (mode == 2 && tris) return f(&rt_hits_kernel<2, true, 1024>, 1024u);
    if (mode == 0 && !tris) return f(&rt_hits_kernel<0, false, 256>, 256u);
    if (mode == 1 && !tris) return f(&rt_hits_kernel<1, false, 1024>, 1024u);
    return hipErrorInvalidValue;
}

// (0 for a (mode, tris) without an instance, as rt_query_threads)
uint32_t rt_hits_threads(int mode, bool tris) {
    uint32_t threads = 0;
    (void)with_hits_instance(mode, tris, [&](auto, uint32_t t) { return threads = t, hipSuccess; });
    return threads;
}

hipError_t rt_hits_occupancy(int mode, bool tris, size_t lds_bytes, int* blocks_per_cu) {
    return with_hits_instance(
        mode, tris, [&](auto kernel, uint32_t t) { return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu); });
}

hipError_t rt_launch_hits(const KernelArgs& ka, int mode, bool tris, size_t lds_bytes, const rtq::QuerySchedule& s,
                          const void* rays, void* hits, void* counts, uint64_t count, uint32_t max_hits, bool pick,
                          unsigned long long* counter, hipStream_t stream) {
    if (s.blocks == 0 || count == 0) return hipSuccess;
    return with_hits_instance(mode, tris, [&](auto kernel, uint32_t t) {
        const HitsArgs qa{static_cast<const float4*>(rays), static_cast<uint4*>(hits), static_cast<uint32_t*>(counts),
                          max_hits,                         pick ? 1u : 0u,            chunk_args(count, counter, s, t)};
        return query_launch_of(kernel, t, s.blocks, lds_bytes, stream, ka, qa);
    });
}
