// nearest.hip -- batched proximity queries for gfx950 (rt_nearest, rt_nearest_device; DESIGN.md
// §5.4n).
//
// rt_nearest_kernel answers "what is the closest surface point to this point?": per point the
// candidate of the smallest key under THE NEAREST-POINT CONTRACT (include/rt_abi.h; the
// operations are rt_nearest_math.h's, which the CPU harness compiles too). The candidates are every
// sphere and every triangle visit of the reference's sweep, boxes disregarded; ties go to
// triangles before spheres, then to the lower sweep position or sphere index.
//
// The kernel stands on the query kernels' frame (rt_query_frame.h): one point per lane, persistent
// wave64s claiming chunks of points from one device counter, ballot + mbcnt refill, the three
// scene placements staged as query.hip stages them. What is its own:
//
//  * The walk instance (kSweep false). The always-tested spheres first, then a stackless skip walk
//    of the triangle accelerator (the quantized nodes of modes 0 and 1 when the scene has them),
//    then one of the sphere BVH. A node is skipped when the certified lower bound of its box
//    (rtn::box_bound: the f32 point-to-box distance, shrunk) is strictly beyond min(best key,
//    max_distance): the bound never exceeds the key of a primitive below the node, so neither the
//    winner nor a tie is ever skipped, whatever the visiting order. Leaves are tested in place.
//  * The visiting order: the octant layouts exist for rays; a point takes the layout of the signs
//    of (root box centre - p), which lists near children first for it. Before the triangle walk a
//    greedy descent to one nearby leaf (near_descend) gives it its limit from the first node on.
//  * The sweep instance (kSweep true): every slot and the reference's sweep over objects and
//    sub-objects, no box read at all. The host launches it in brute-force mode, with tuning
//    "nearest_walk" 0, and while the sub-object boxes are not known to enclose their triangles.
//  * The slots hold r * r; the key needs |r| as uploaded, which a leaf reads from a table by
//    original index (NearestArgs::radius, global memory in every placement).
//  * A lane keeps the winner's identity only (key, order key, three words); the record is rebuilt
//    from it when the search ends.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
#include "rt_nearest_math.h"
#include "rt_path_common.h"
#include "rt_query_frame.h"

#pragma clang fp contract(off)

using namespace rtk;

struct NearestArgs {
    const float4* __restrict__ points;  // rt_near_point[count]: position.xyz, max_distance
    uint4* out;                         // rt_nearest[count]
    const float* __restrict__ radius;   // |radius| as uploaded, by original sphere index
    uint32_t descend;                   // 1: a greedy descent to one leaf before the triangle walk (tuning "nearest_walk" 1)
    ChunkArgs chunks;                   // every chunk is claimed: first_chunk and claimed_from are 0
};

namespace {

// A lane's search: the point, the best candidate so far and the walk's position.
struct NearSearch {
    rtn::V3 p;
    float max_distance;
    float best;        // the best key so far (+inf: none)
    uint32_t order;    // its order key (rtn::kNoOrder: none)
    uint32_t a, b, c;  // sphere: slot; triangle: triangle, object, sub-object
    float limit;       // min(best, max_distance): what a box bound must exceed to cull
    uint32_t node, phase;  // phase 0: triangle accelerator, 1: sphere BVH, 2: done
};

__device__ __forceinline__ rtn::V3 rv(float4 v) { return rtn::v3(v.x, v.y, v.z); }

__device__ __forceinline__ void offer(NearSearch& s, float key, uint32_t order, uint32_t a, uint32_t b, uint32_t c) {
    if (!rtn::candidate_wins(key, order, s.max_distance, s.best, s.order)) return;
    s.best = key;
    s.order = order;
    s.a = a;
    s.b = b;
    s.c = c;
    s.limit = fminf(key, s.max_distance);
}

__device__ __forceinline__ void near_sphere(const SceneView& sv, const NearestArgs& na, uint32_t slot, NearSearch& s) {
    const uint32_t orig = sv.orig[slot];
    if (orig == 0xffffffffu) return;  // a padding slot (sphere_bvh.h)
    float l;
    const float key = rtn::sphere_key(rv(sv.sph[slot]), na.radius[orig], s.p, l);
    offer(s, key, rtn::kSphereOrder + orig, slot, 0u, 0u);
}

__device__ __forceinline__ void near_triangle(const KernelArgs& ka, uint32_t ti, uint32_t seq, uint32_t obj,
                                              uint32_t sub, NearSearch& s) {
    const TriGeom g = load_tri(ka.triangles, ti);
    const rtn::TriNearest t = rtn::tri_nearest(rtn::v3(g.a.x, g.a.y, g.a.z), rtn::v3(g.ab.x, g.ab.y, g.ab.z),
                                               rtn::v3(g.ac.x, g.ac.y, g.ac.z), s.p);
    offer(s, rtn::point_key(t.q, s.p), seq, ti, obj, sub);
}

// Every triangle of one (object, sub-object) pair of the sweep, from sweep position `seq` on.
__device__ __forceinline__ void near_sub_object(const SceneView& sv, const KernelArgs& ka, uint32_t obj, uint32_t si,
                                                uint32_t seq, NearSearch& s) {
    const RtSubObject sub = sv.sub[si];
    for (uint32_t j = 0; j < sub.triangle_count; ++j)
        near_triangle(ka, min(sub.first_triangle_index + j, ka.triangle_count - 1u), seq + j, obj, si, s);
}

// The reference's sweep order (check_triangles, :422-517) with its index clamps, boxes disregarded.
__device__ __forceinline__ void near_sweep_triangles(const SceneView& sv, const KernelArgs& ka, NearSearch& s) {
    uint32_t seq = 0u;
    for (uint32_t oi = 0; oi < ka.object_count; ++oi) {
        const RtObject& ob = sv.obj[oi];
        const uint32_t first_sub = ob.first_sub_object_index, n_sub = ob.sub_object_count;
        for (uint32_t i = 0; i < n_sub; ++i) {
            const uint32_t si = min(first_sub + i, ka.sub_object_count - 1u);
            near_sub_object(sv, ka, oi, si, seq, s);
            seq += sv.sub[si].triangle_count;
        }
    }
}

// The layout whose order lists near children first for p (rtn::point_octant), from a root's box.
__device__ __forceinline__ uint32_t point_octant(float4 lo, float4 hi, rtn::V3 p) {
    return rtn::point_octant(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, p);
}

__device__ __forceinline__ void tri_node_at(const SceneView& sv, uint32_t node, float4& lo, float4& hi) {
    if (sv.tri_q) {
        qnode_decode(sv, sv.tri_q[node], node, lo, hi);
    } else {
        lo = sv.tri_nodes[2u * node];
        hi = sv.tri_nodes[2u * node + 1u];
    }
}

// A node of the hierarchy of the current walk.
template <bool kTris>
__device__ __forceinline__ void near_node_at(const SceneView& sv, bool tri, uint32_t node, float4& lo, float4& hi) {
    if (kTris && tri) {
        tri_node_at(sv, node, lo, hi);
    } else {
        lo = sv.nodes[2u * node];
        hi = sv.nodes[2u * node + 1u];
    }
}

__device__ __forceinline__ float near_bound(const SceneView& sv, const KernelArgs& ka, bool tri, float4 lo, float4 hi,
                                            const NearSearch& s) {
    const float abs_part = tri ? rtn::tri_abs_part(sv.tri_extent) : rtn::sphere_abs_part(ka.sphere_extent);
    return rtn::box_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, s.p, abs_part);
}

// The primitives of a leaf record: a sub-object's triangles, or an aligned group of 4 sphere slots.
template <bool kTris>
__device__ __forceinline__ void near_leaf(const SceneView& sv, const KernelArgs& ka, const NearestArgs& na, bool tri,
                                          uint32_t leaf, NearSearch& s) {
    if (kTris && tri) {
        const uint4 pr = sv.tri_prims[leaf & 0xffffffu];  // object, sub-object, seq_base, range
        near_sub_object(sv, ka, pr.x, pr.y, pr.z, s);
    } else {
        const uint32_t slot = leaf & 0xffffffu;
        for (uint32_t k = 0; k < 4u; ++k) near_sphere(sv, na, slot + k, s);
    }
}

// The greedy descent before a walk: from the layout's root to one leaf, at every internal node into
// the child of the smaller bound (the children of node n are n + 1 and the node that n + 1's skip
// link names), and that leaf's primitives are tested. It only adds candidates, so the result is
// the walk's; what it gives the walk is a limit from a nearby leaf before the first node, where the
// skip walk alone keeps max_distance until the layout's order happens to reach something close.
// `end`: the hierarchy's node count; at most 64 levels (a deeper tree just gets no head start).
template <bool kTris>
__device__ __forceinline__ void near_descend(const SceneView& sv, const KernelArgs& ka, const NearestArgs& na, bool tri,
                                             uint32_t root, uint32_t end, NearSearch& s) {
    uint32_t node = root;
    for (uint32_t depth = 0; depth < 64u && node < end; ++depth) {
        float4 lo, hi;
        near_node_at<kTris>(sv, tri, node, lo, hi);
        const uint32_t leaf = __float_as_uint(hi.w);
        if (leaf != 0xffffffffu) {
            near_leaf<kTris>(sv, ka, na, tri, leaf, s);
            return;
        }
        const uint32_t left = node + 1u;
        if (left >= end) return;
        float4 llo, lhi;
        near_node_at<kTris>(sv, tri, left, llo, lhi);
        const uint32_t right = __float_as_uint(llo.w);
        node = left;
        if (right > left && right < end) {
            float4 rlo, rhi;
            near_node_at<kTris>(sv, tri, right, rlo, rhi);
            if (near_bound(sv, ka, tri, rlo, rhi, s) < near_bound(sv, ka, tri, llo, lhi, s)) node = right;
        }
    }
}

// Starts the walk of `phase` (or the next one that has nodes).
template <bool kTris>
__device__ __forceinline__ void near_phase(const SceneView& sv, const KernelArgs& ka, const NearestArgs& na,
                                           uint32_t phase, NearSearch& s) {
    if (kTris && phase == 0u && ka.tri_accel && ka.tri_nodes != 0u) {
        float4 lo, hi;
        tri_node_at(sv, 0u, lo, hi);
        s.node = point_octant(lo, hi, s.p) * ka.tri_octant_stride;
        s.phase = 0u;
        if (na.descend) near_descend<kTris>(sv, ka, na, true, s.node, ka.tri_nodes, s);
        return;
    }
    if (ka.sphere_nodes != 0u) {
        s.node = point_octant(sv.nodes[0], sv.nodes[1], s.p) * ka.sphere_octant_stride;
        s.phase = 1u;  // (no descent here: on the sphere BVH it cost more than it saved)
        return;
    }
    s.phase = 2u;
}

// The search of a lane that took a point: what is tested without a walk, then the first walk.
template <bool kTris, bool kSweep>
__device__ __forceinline__ void near_begin(const SceneView& sv, const KernelArgs& ka, const NearestArgs& na,
                                           NearSearch& s) {
    s.best = __builtin_inff();
    s.order = rtn::kNoOrder;
    s.a = s.b = s.c = 0u;
    s.limit = s.max_distance;
    s.node = 0u;
    if constexpr (kSweep) {
        if constexpr (kTris) near_sweep_triangles(sv, ka, s);
        for (uint32_t i = 0; i < ka.sphere_slot_count; ++i) near_sphere(sv, na, i, s);
        s.phase = 2u;
    } else {
        for (uint32_t i = 0; i < ka.sphere_always; ++i) near_sphere(sv, na, i, s);
        if constexpr (kTris)
            if (!ka.tri_accel) near_sweep_triangles(sv, ka, s);  // (tuning "tri_bvh" 0: no accelerator to walk)
        near_phase<kTris>(sv, ka, na, 0u, s);
    }
}

// One node of the current walk. Skip links only advance, so the walk terminates on any input.
template <bool kTris>
__device__ __forceinline__ void near_step(const SceneView& sv, const KernelArgs& ka, const NearestArgs& na,
                                          NearSearch& s) {
    const bool tri = kTris && s.phase == 0u;
    float4 lo, hi;
    near_node_at<kTris>(sv, tri, s.node, lo, hi);
    const bool enter = !rtn::bound_culls(near_bound(sv, ka, tri, lo, hi, s), s.limit);
    const uint32_t leaf = __float_as_uint(hi.w);
    const bool at_leaf = enter && leaf != 0xffffffffu;
    if (at_leaf) near_leaf<kTris>(sv, ka, na, tri, leaf, s);
    s.node = (enter && !at_leaf) ? s.node + 1u : __float_as_uint(lo.w);
    if (tri) {
        if (s.node >= ka.tri_nodes) near_phase<kTris>(sv, ka, na, 1u, s);
    } else if (s.node >= ka.sphere_nodes) {
        s.phase = 2u;
    }
}

// The 64-byte record of the winner, rebuilt from its identity by the contract's operations.
template <bool kTris>
__device__ __forceinline__ void write_nearest(const SceneView& sv, const KernelArgs& ka, const NearestArgs& na,
                                              const NearSearch& s, uint4* rec) {
    if (s.order == rtn::kNoOrder) {
        rec[0] = make_uint4(__float_as_uint(rtn::kMissDistance), 0u, 0u, 0u);
        rec[1] = rec[2] = rec[3] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    rtn::V3 q, n;
    uint32_t feature, kind, index, sub = 0u, tri = 0u, material, side;
    if (s.order >= rtn::kSphereOrder) {
        const uint32_t orig = s.order - rtn::kSphereOrder;
        const rtn::SphereNearest r = rtn::sphere_nearest(rv(sv.sph[s.a]), na.radius[orig], s.p);
        q = r.point;
        n = r.normal;
        feature = 0u;
        kind = RT_HIT_SPHERE;
        index = orig;
        material = sv.sph_mat[orig];
        side = r.side;
    } else {
        const RtTriangleHot& t = ka.triangles[s.a];
        const TriGeom g = load_tri(ka.triangles, s.a);
        const rtn::V3 a = rtn::v3(g.a.x, g.a.y, g.a.z);
        const rtn::TriNearest r = rtn::tri_nearest(a, rtn::v3(g.ab.x, g.ab.y, g.ab.z), rtn::v3(g.ac.x, g.ac.y, g.ac.z), s.p);
        q = r.q;
        n = rtn::v3(t.fn.x, t.fn.y, t.fn.z);
        feature = r.feature;
        kind = RT_HIT_TRIANGLE;
        index = s.b;
        sub = s.c;
        tri = s.a;
        material = kTris ? sv.obj[s.b].material_index : 0u;
        side = rtn::dot(rtn::v3(g.cn.x, g.cn.y, g.cn.z), s.p - a) >= 0.0f ? 1u : 0u;
    }
    rec[0] = make_uint4(__float_as_uint(s.best), __float_as_uint(q.x), __float_as_uint(q.y), __float_as_uint(q.z));
    rec[1] = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), feature);
    rec[2] = make_uint4(kind, index, sub, tri);
    rec[3] = make_uint4(material, side, 0u, 0u);
}

}  // namespace

template <int kMode, bool kTris, bool kSweep, uint32_t kThreads>
__global__ void __launch_bounds__(kThreads, 1) rt_nearest_kernel(KernelArgs ka, NearestArgs na) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // The closest-hit query's image (query.hip): what the search and the record read.
    SceneView sv = global_scene_view<kMode, kTris>(ka, nullptr);
    if constexpr (kMode >= 1) {
        sv = stage_walk_tables<kTris, kThreads>(ka, lds, sv);
        sv = stage_sphere_materials<kThreads>(ka, lds, sv);
    }
    if constexpr (kMode == 2) sv = stage_triangle_tables<kThreads>(ka, lds, sv);
    if constexpr (kMode >= 1) __syncthreads();

    uint32_t mode = kLaneIdle;
    unsigned long long item = 0;
    NearSearch s{};
    s.phase = 2u;

    // Every chunk comes from the counter, as in the closest-hit kernel.
    WaveChunk c{0, 0, false, false};
    claim_chunk<false>(na.chunks, 0u, c);

    while (true) {
        // 1. The records of the lanes whose search has finished.
        if (mode == kLaneDone) {
            write_nearest<kTris>(sv, ka, na, s, na.out + 4ull * item);
            mode = kLaneIdle;
        }
        // 2. Refill: idle lanes take the chunk's next points, in order.
        while (true) {
            const uint64_t need = __ballot(mode == kLaneIdle);
            if (need == 0 || c.dry) break;
            const uint32_t avail = (uint32_t)(c.end - c.next);
            if (mode == kLaneIdle) {
                const uint32_t rank = rank_among(need);
                if (rank < avail) {
                    item = c.next + rank;
                    const float4 r = na.points[item];
                    s.p = rtn::v3(r.x, r.y, r.z);
                    s.max_distance = r.w;
                    mode = kLaneSetup;
                }
            }
            c.next += min((uint32_t)__popcll(need), avail);
            if (c.next == c.end) claim_chunk<false>(na.chunks, 0u, c);
        }
        // 3. Start the search of every lane that took a point. A max_distance that is NaN or
        // negative admits no candidate: the search is skipped.
        if (mode == kLaneSetup) {
            mode = kLaneDone;
            s.best = __builtin_inff();
            s.order = rtn::kNoOrder;
            s.phase = 2u;
            if (s.max_distance >= 0.0f) {
                near_begin<kTris, kSweep>(sv, ka, na, s);
                if (s.phase != 2u) mode = kLaneTrav;
            }
        }
        if (__ballot(mode != kLaneIdle) == 0 && c.dry) break;
        // 4. Walk in blocks of node steps until at most trav_threshold lanes still do (finished
        // lanes are then written and refilled together), or to the end once no points are left.
        if constexpr (!kSweep) {
            const uint32_t thresh = c.dry ? 0u : ka.trav_threshold;
            while (true) {
                const uint32_t n_trav = (uint32_t)__popcll(__ballot(mode == kLaneTrav));
                if (n_trav <= thresh || n_trav == 0u) break;
#pragma unroll 1
                for (int k = 0; k < 4; ++k) {
                    if (mode == kLaneTrav) {
                        near_step<kTris>(sv, ka, na, s);
                        if (s.phase == 2u) mode = kLaneDone;
                    }
                }
            }
        }
    }
}

// The instances, (mode, triangles, sweep, threads): f(kernel, threads) for the one asked for. The
// workgroup sizes are the closest-hit query's (query.hip).
template <class F>
static hipError_t with_nearest_instance(int mode, bool tris, bool sweep, F f) {
    if (sweep) {
        if (mode == 0 && tris) return f(&rt_nearest_kernel<0, true, true, 256>, 256u);
        if (mode == 1 && tris) return f(&rt_nearest_kernel<1, true, true, 1024>, 1024u);
        if (mode == 2 && tris) return f(&rt_nearest_kernel<2, true, true, 1024>, 1024u);
        if (mode == 0 && !tris) return f(&rt_nearest_kernel<0, false, true, 256>, 256u);
        if (mode == 1 && !tris) return f(&rt_nearest_kernel<1, false, true, 1024>, 1024u);
        return hipErrorInvalidValue;
    }
    if (mode == 0 && tris) return f(&rt_nearest_kernel<0, true, false, 256>, 256u);
    if (mode == 1 && tris) return f(&rt_nearest_kernel<1, true, false, 1024>, 1024u);
    if (mode == 2 && tris) return f(&rt_nearest_kernel<2, true, false, 1024>, 1024u);
    if (mode == 0 && !tris) return f(&rt_nearest_kernel<0, false, false, 256>, 256u);
    if (mode == 1 && !tris) return f(&rt_nearest_kernel<1, false, false, 1024>, 1024u);
    return hipErrorInvalidValue;
}

// (0 for a (mode, tris) without an instance, as rt_query_threads; the same for both instances)
uint32_t rt_nearest_threads(int mode, bool tris) {
    uint32_t threads = 0;
    (void)with_nearest_instance(mode, tris, false, [&](auto, uint32_t t) { return threads = t, hipSuccess; });
    return threads;
}

hipError_t rt_nearest_occupancy(int mode, bool tris, bool sweep, size_t lds_bytes, int* blocks_per_cu) {
    return with_nearest_instance(mode, tris, sweep, [&](auto kernel, uint32_t t) {
        return query_occupancy_of(kernel, t, lds_bytes, blocks_per_cu);
    });
}

hipError_t rt_launch_nearest(const KernelArgs& ka, int mode, bool tris, bool sweep, size_t lds_bytes,
                             const rtq::QuerySchedule& s, const void* points, void* out, const float* radius,
                             bool descend, uint64_t count, unsigned long long* counter, hipStream_t stream) {
    if (s.blocks == 0 || count == 0) return hipSuccess;
    return with_nearest_instance(mode, tris, sweep, [&](auto kernel, uint32_t t) {
        const NearestArgs na{static_cast<const float4*>(points), static_cast<uint4*>(out), radius,
                             descend ? 1u : 0u, chunk_args(count, counter, s, t)};
        return query_launch_of(kernel, t, s.blocks, lds_bytes, stream, ka, na);
    });
}
